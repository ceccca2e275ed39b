// CylinderTag.h -- C++ host layer with the reference's class interface on top of the C ABI (include/ctag.h).
//
// Mirrors /root/reference/header/CylinderTag.h:12-52 and the structs of header/corner_detector.h:10-22 for the
// detection path: same class name, constructor forms, detect() signature, MarkerInfo field names, the same
// `throw std::string` error behaviour of the loaders (CylinderTag.cpp:21,39,51,61) and the same two stdout
// messages with untouched output on the early returns (CylinderTag.cpp:87-96).  loadModel / loadCamera / estimatePose
// (header/CylinderTag.h:24-30, CylinderTag.cpp:161-209) are here too, on the GPU pose back end of include/ctag_pose.h
// (EPnP + LM per marker, k_pose.hip), and so is drawAxis (header/CylinderTag.h:33, CylinderTag.cpp:211-246) on the overlay
// of k_draw.hip: the image the reference would imshow is kept in the object (axisImage()).
//
// Build with -DCTAG_WITH_OPENCV to use cv::Mat / cv::Point2f / cv::Mat1i (drop-in next to the reference's
// pose_estimation.cpp); without it a minimal stand-alone Mat / Point2f is used (this image has no OpenCV).
#pragma once
#ifndef CYLINDERTAG_AMD_H
#define CYLINDERTAG_AMD_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#ifdef CTAG_WITH_OPENCV
#include <opencv2/core.hpp>
namespace ctag_host {
using cv::Mat;
using cv::Mat1i;
using cv::Point2f;
using cv::Point3f;
}  // namespace ctag_host
#else
namespace ctag_host {
struct Point2f {
    float x = 0.f, y = 0.f;
    Point2f() = default;
    Point2f(float x_, float y_) : x(x_), y(y_) {}
};
struct Point3f {
    float x = 0.f, y = 0.f, z = 0.f;
    Point3f() = default;
    Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
// borrowed 8-bit image view (what detect() needs from cv::Mat): one channel (gray) or three (BGR, as a camera delivers it)
struct Mat {
    int rows = 0, cols = 0;
    size_t step = 0;  // bytes per row
    const unsigned char* data = nullptr;
    int nch = 1;
    Mat() = default;
    Mat(int r, int c, const unsigned char* d, size_t s = 0, int ch = 1) : rows(r), cols(c), step(s ? s : (size_t)c * ch), data(d), nch(ch) {}
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
    int channels() const { return nch; }
};
// dictionary matrix (what the reference takes as cv::Mat1i)
struct Mat1i {
    int rows = 0, cols = 0;
    std::vector<int> v;
    Mat1i() = default;
    Mat1i(int r, int c) : rows(r), cols(c), v((size_t)r * c, 0) {}
    int& operator()(int i, int j) { return v[(size_t)i * cols + j]; }
    int operator()(int i, int j) const { return v[(size_t)i * cols + j]; }
};
}  // namespace ctag_host
#endif

struct ctag_handle;
struct ctag_params;  // include/ctag_types.h: the detector's tunables (the reference's member constants, header/corner_detector.h:90-144)
struct ctag_track_opts;  // include/ctag_pose.h: the options of smoothRigTrack
struct ctag_track_filter;       // ... the live filter behind startRigTracking / trackRigs / predictRigs
struct ctag_track_filter_opts;  // ... and its options
struct ctag_track_noise_opts;   // ... the options of calibrateTrackNoise
struct ctag_hand_eye_opts;  // include/ctag_pose.h: the options of calibrateHandEye

// reference: header/corner_detector.h:16-22
struct MarkerInfo {
    int markerID = -1;
    std::vector<int> featurePos, feature_ID, feature_ID_left, feature_ID_right;
    std::vector<std::vector<ctag_host::Point2f>> cornerLists;
    std::vector<ctag_host::Point2f> feature_center;
    std::vector<float> edge_length, cr_left, cr_right;
};

// reference: header/pose_estimation.h:12-25.  With OpenCV the matrices are cv::Mat exactly as in the reference
// (Intrinsic / distCoeffs CV_32F as cameraParams.yml stores them, rvec / tvec 3x1 CV_64F as solvePnP creates them);
// without it plain arrays of the same element types.
#ifdef CTAG_WITH_OPENCV
struct CamInfo {
    cv::Mat Intrinsic, distCoeffs;
};
struct PoseInfo {
    int markerID;
    cv::Mat rvec, tvec;
};
// one pose per rig of markers (new): the pose of the rig's common model frame, members = indices into the marker list
struct RigPoseInfo {
    int rigID;
    cv::Mat rvec, tvec;
    std::vector<int> members;
    std::vector<std::pair<int, int>> viewMembers;  // estimateMultiViewRigPose: (camera, index into that camera's marker list)
};
// pose of one camera in the reference frame of a camera set (new): X_cam = R(rvec) X_ref + tvec, both 3x1 CV_64F
struct ViewPose {
    cv::Mat rvec, tvec;
};
#else
struct CamInfo {
    float Intrinsic[9] = {0};       // row-major 3x3
    std::vector<float> distCoeffs;  // k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]
};
struct PoseInfo {
    int markerID = -1;
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
};
struct RigPoseInfo {
    int rigID = -1;
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
    std::vector<int> members;
    std::vector<std::pair<int, int>> viewMembers;  // estimateMultiViewRigPose: (camera, index into that camera's marker list)
};
// pose of one camera in the reference frame of a camera set (new): X_cam = R(rvec) X_ref + tvec
struct ViewPose {
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
};
#endif
// covariance and residual diagnostics of one per-marker pose (new): the fields of ctag_pose_cov_rec (include/ctag_pose.h, pose
// covariance) for the PoseInfo with the same markerID at the same place of estimatePose's list
struct PoseCovInfo {
    int markerID = -1;
    int status = 0;  // CTAG_COV_*; every other field is 0 unless it is CTAG_COV_OK
    int nPoints = 0, dof = 0, worstPoint = 0, nOutliers = 0;
    double cost = 0, sigma2Hat = 0, sigma2Used = 0, maxResidualPx = 0, minPivot = 0;
    double cov[36] = {0};  // row-major 6x6: rows / columns 0-2 rotation (rad), 3-5 translation (model units)
};
// one per-marker pose minimised again under a loss (new): the fields of ctag_robust_pose_rec (include/ctag_pose.h, robust refit) for the
// PoseInfo with the same markerID at the same place of estimatePose's list
struct RobustPoseInfo {
    int markerID = -1;
    int status = 0;  // CTAG_ROBUST_*; every other field is 0 unless it is CTAG_ROBUST_OK
    int nPoints = 0, nInliers = 0, iterations = 0, loss = 0, worstPoint = 0;
    std::vector<bool> inlier;  // nPoints entries, in the correspondence builder's point order
    double scalePx = 0, sigmaHat = 0, costLs0 = 0, costLs = 0, cost0 = 0, cost = 0, maxResidualPx = 0;
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};  // the refitted pose
};
// one frame of a rig's smoothed track (new): the fields of ctag_track_rec (include/ctag_pose.h, track smoothing)
struct TrackInfo {
    int rigID = -1;
    int status = 0;  // CTAG_TRACK_*; the fields below are 0 unless it is CTAG_TRACK_OK or CTAG_TRACK_SINGULAR
    bool measured = false, downweighted = false;
    bool gated = false, started = false;              // the track filter's flags (trackRigs); false from smoothRigTrack
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};  // the smoothed pose, in the frame of the input poses
    double w[3] = {0, 0, 0}, v[3] = {0, 0, 0};        // angular (rad / s) and translational (model units / s) velocity
    double cov[36] = {0};                             // row-major 6x6 of the pose, tangent parametrisation
    double velSigma[6] = {0};
    double mahalanobis2 = 0, weight = 0;
};
// the filter's noise levels fitted from a recorded track (new): the fields of ctag_track_noise_rec (include/ctag_pose.h, track noise fit)
struct TrackNoiseInfo {
    int rigID = -1;    // -1 for the pooled search
    int status = 0;    // CTAG_NOISE_*
    int nTerms = 0, nFree = 0, rounds = 0;
    unsigned flags = 0;  // CTAG_NOISE_FLAG_EDGE << axis
    double qRot = 0, qTrans = 0, covScale = 1;
    double log2Sigma[3] = {0, 0, 0};
    double score = 0, scoreStart = 0, meanM2 = 0;
};
// a robot's link pose in one frame, base <- gripper (new): X_out = R(rvec) X_in + tvec; a non-finite entry drops the frame
struct LinkPose {
    double rvec[3] = {0, 0, 0}, tvec[3] = {0, 0, 0};
};
// one frame of one rig's hand-eye problem (new): the fields of ctag_hand_eye_frame_rec (include/ctag_pose.h, hand-eye calibration)
struct HandEyeFrameInfo {
    int status = 0;
    bool used = false, downweighted = false;
    double e[6] = {0};  // the residual at the returned state: rotation, translation
    double mahalanobis2 = 0, weight = 0;
};
// the two fixed transforms of one rig's hand-eye problem (new): the fields of ctag_hand_eye_rec
struct HandEyeInfo {
    int rigID = -1;
    int status = 0;  // CTAG_HE_*
    int nUsed = 0, nDownweighted = 0, rounds = 0, dof = 0;
    LinkPose P, Q;   // mode 0: camera <- gripper, base <- rig; mode 1: camera <- base, gripper <- rig
    double cost0 = 0, cost = 0, lambda = 0, sigma2Hat = 0, minPivot = 0;
    double cov[144] = {0};  // row-major 12x12: P's rotation and translation, then Q's
    std::vector<HandEyeFrameInfo> frames;  // one per frame
};
// the annotated frame of drawAxis: rows x cols pixels of 3 bytes, channel c = Scalar component c (imgMark in the reference)
struct AxisImage {
    int rows = 0, cols = 0;
    std::vector<unsigned char> px;  // rows * cols * 3, top-down
};
struct ModelInfo {
    int MarkerID = -1;
    ctag_host::Point3f axis, base;
    std::vector<ctag_host::Point3f> corners;
};

class CylinderTag {
   public:
    // Load state matrix of CylinderTag from file (reference: CylinderTag.cpp:6-9, 16-41)
    // `params` (optional, new): tunables other than the reference's constants -- what a maintainer would otherwise edit in
    // header/corner_detector.h:90,110,122,135-137,144 -- see ctag_params_default / ctag_create_ex in include/ctag.h
    CylinderTag(const std::string& path, int device_id = 0, const ctag_params* params = nullptr);
    // Manual input of the state matrix (reference: CylinderTag.cpp:11-14, 43-54).  The reference leaves
    // featureSize unset on this path; it must be given here (default 2 as in CTag_2f12c).
    CylinderTag(const ctag_host::Mat1i& set_state, int feature_size = 2, int device_id = 0, const ctag_params* params = nullptr);
    ~CylinderTag();
    CylinderTag(const CylinderTag&) = delete;
    CylinderTag& operator=(const CylinderTag&) = delete;

    // Marker Detector (reference: header/CylinderTag.h:21, CylinderTag.cpp:67-159).  A three-channel image is taken as the BGR frame the
    // reference's caller would have passed through cvtColor(BGR2GRAY) first (main.cpp:36,54): that conversion then runs on the device.
    void detect(const ctag_host::Mat& img, std::vector<MarkerInfo>& cornerList, int adaptiveThresh = 5,
                const bool cornerSubPix = false, int cornerSubPixDist = 3);

    // Batch form (new): n frames of identical size, frame i at frames + i*frame_stride; one vector per frame.
    // status[i] is CTAG_OK / CTAG_NO_CORNER / CTAG_NO_FEATURE / error; lists[i] is assigned only on CTAG_OK.
    void detectBatch(const unsigned char* frames, int n, int rows, int cols, size_t row_stride, size_t frame_stride,
                     std::vector<std::vector<MarkerInfo>>& lists, std::vector<int>& status, int adaptiveThresh = 5,
                     const bool cornerSubPix = false, int cornerSubPixDist = 3);

    // Load the reconstructed marker models / the camera (reference: header/CylinderTag.h:24,27; CylinderTag.cpp:161-196;
    // both throw std::string when the file cannot be read)
    void loadModel(const std::string& path, std::vector<ModelInfo>& reconstruct_model);
    void loadCamera(const std::string& path, CamInfo& camera);

    // Reconstruct the marker models themselves (new; include/ctag_pose.h, model reconstruction: ctag_model_fit).  framesOfMarkers[f] is what
    // detect() returned for frame f of a sequence that shows the objects (a few dozen to a few thousand frames); seedModel is a rough model --
    // an ideal cylinder of nominal radius, or an older model -- whose model size is the dictionary's column count.  outModel is the model that
    // minimises the reprojection error over all frames, in the seed's frame and scale; stripHeight > 0 rescales it so that the strips'
    // vertical edges have that length.  Models no frame shows come back as the seed.  A frame must fit one detection record (<= 100 markers,
    // <= 100 features, as detect() returns them).  Throws std::string on error.
    void reconstructModel(const std::vector<std::vector<MarkerInfo>>& framesOfMarkers, const std::vector<ModelInfo>& seedModel, CamInfo camera,
                          std::vector<ModelInfo>& outModel, double stripHeight = 0.0);
    // Carry the models of every rig into ONE frame (new; include/ctag_pose.h, rig assembly: ctag_rig_fit).  reconstructModel returns each
    // model in its own frame; estimateRigPose needs the models of a rig in one.  framesOfMarkers[f] is what detect() returned for frame f of
    // a sequence that shows two or more markers of a rig together; rigOfModel[i] is the rig of model i (-1: none).  outModel has the models
    // of each rig in the frame of the rig's anchor; placedRigOfModel is rigOfModel with the models the frames never linked to their rig at
    // -1 (they keep their corners): pass it, not rigOfModel, to estimateRigPose.  Throws std::string on error.
    void assembleRigModel(const std::vector<std::vector<MarkerInfo>>& framesOfMarkers, const std::vector<ModelInfo>& model,
                          const std::vector<int>& rigOfModel, CamInfo camera, std::vector<ModelInfo>& outModel, std::vector<int>& placedRigOfModel);
    // Fit the poses of the cameras of a set from detections they share (new; include/ctag_pose.h, camera set fit: ctag_camera_fit with
    // the defaults).  markersPerCamera[c][f] is what camera c's detect() returned at instant f -- the same f is the same instant in every
    // camera -- while a rig of rigOfModel is carried through the volume the cameras watch; cameras[c] are the intrinsics, which stay as
    // given.  cameraPoses[c] is camera c's pose in the frame of the anchor camera (the lowest-numbered camera that shares enough instants
    // with another; its pose is zero): what estimateMultiViewRigPose takes.  placed[c] is 0 for a camera the instants never linked to the
    // others (its pose is zero and means nothing).  Returns whether every camera was placed.  Throws std::string on error.
    bool calibrateCameraSet(const std::vector<std::vector<std::vector<MarkerInfo>>>& markersPerCamera, const std::vector<ModelInfo>& model,
                            const std::vector<int>& rigOfModel, const std::vector<CamInfo>& cameras, std::vector<ViewPose>& cameraPoses,
                            std::vector<int>& placed);
    // Fit the camera itself from views of rigs whose models are known (new; include/ctag_pose.h, intrinsics fit: ctag_intrinsics_fit with
    // the defaults but freeMask and tieFocal).  markersPerFrame[f] is what detect() returned for view f of a sequence that carries a rig of
    // rigOfModel (empty: every model a rig of its own) through the whole image at several distances and tilts; seed is a rough camera --
    // the focal length off by several per cent, the principal point by tens of pixels, no distortion will do -- whose number of
    // distortion coefficients is the result's.  camera is the fitted camera (its matrices are float, as cameraParams.yml stores them); sigma, if given, gets the sixteen standard deviations
    // fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (0 for a parameter that was not fitted): look at them, a single small marker cannot
    // fix a principal point and they say so.  freeMask: bit i = parameter i is fitted, 0 = fx fy cx cy and every coefficient the seed
    // has; tieFocal: fy = fx x (seed fy / seed fx).  Returns whether a camera was fitted (false: no usable view, too few points, or a
    // degenerate set; camera is the seed then).  Models and rig layout stay as given: alternate with reconstructModel /
    // assembleRigModel.  Throws std::string on error.
    bool calibrateCamera(const std::vector<std::vector<MarkerInfo>>& markersPerFrame, const std::vector<ModelInfo>& model, const std::vector<int>& rigOfModel,
                         CamInfo seed, CamInfo& camera, std::vector<double>* sigma = nullptr, unsigned freeMask = 0, bool tieFocal = false);
    // Write a model list in the text format loadModel reads (CylinderTag.cpp:168-188), floats with 9 significant digits: loadModel gives
    // back the same values bit for bit.  Throws std::string when the file cannot be written.
    void saveModel(const std::string& path, const std::vector<ModelInfo>& model);

    // Estimate the pose of the markers (reference: header/CylinderTag.h:30, CylinderTag.cpp:198-209): one PoseInfo per
    // marker that has a model, PoseInfo::markerID = index into reconstruct_model (pose_estimation.cpp:59,69).
    // useDensePoseRefine is accepted and ignored: the reference's DenseSolver is empty (pose_estimation.cpp:145-148).
    void estimatePose(const ctag_host::Mat& img, std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, CamInfo camera,
                      std::vector<PoseInfo>& pose, bool useDensePoseRefine = false);
    // Covariance of estimatePose's poses (new; ctag_estimate_pose_cov): the poses are estimated again from `markers`, and covariance[i]
    // describes the pose estimatePose returns at place i (markers without a model are erased in both).  tangent: the unknowns are
    // R <- Exp(dw) R, t <- t + dt with dw in the camera frame (CTAG_COV_PARAM_TANGENT), else (rvec, tvec) themselves; sigmaPx > 0:
    // the pixel noise to assume, else the residuals' own estimate; outlierK as ctag_cov_opts::outlier_k.
    void estimatePoseCovariance(std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, CamInfo camera,
                                std::vector<PoseCovInfo>& covariance, bool tangent = true, double sigmaPx = 0.0, double outlierK = 3.0);

    // estimatePose's poses minimised again under a loss (new; ctag_estimate_pose_robust): the poses are estimated again from `markers`,
    // and robust[i] refits the pose estimatePose returns at place i (markers without a model are erased in both).  cauchy: Ceres'
    // CauchyLoss, else HuberLoss, per point; scalePx > 0: the loss's scale, else 2.5 x the residuals' own median-based sigma, at least
    // 0.05 px; maxIterations 0 .. 50 (0: evaluate the source pose only).
    void estimatePoseRobust(std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, CamInfo camera,
                            std::vector<RobustPoseInfo>& robust, bool cauchy = true, double scalePx = 0.0, int maxIterations = 50);

    // One pose per rig of markers (new; include/ctag_pose.h, ctag_estimate_rig_pose): rigOfModel[i] is the rig of model i (-1: none,
    // rigs 0 .. max), the models of one rig share one frame.  The pose of a rig is EPnP + PoseBA over the union of its member
    // markers' correspondences; RigPoseInfo::members lists the members as indices into `markers`.  Rigs with no member in the
    // list are erased (as estimatePose erases markers without a model).  `markers` must fit one detection record (<= 100 markers,
    // <= 100 features, as detect() returns them).  Throws std::string on error or on a rig whose points do not give a pose.
    void estimateRigPose(std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, const std::vector<int>& rigOfModel,
                         CamInfo camera, std::vector<RigPoseInfo>& pose);

    // One pose per rig from several calibrated cameras that saw the same instant (new; include/ctag_pose.h,
    // ctag_estimate_mv_rig_pose): markersPerCamera[c] is camera c's marker list, cameras[c] / cameraPoses[c] its intrinsics and its
    // pose in the reference frame (1 .. 8 cameras).  The pose of a rig maps its model frame into the REFERENCE frame.  Follows
    // estimateRigPose: rigs no camera sees are erased, std::string is thrown on error or on a rig whose points do not give a pose;
    // RigPoseInfo::viewMembers lists the members as (camera, marker index) pairs and `members` stays empty.
    void estimateMultiViewRigPose(const std::vector<std::vector<MarkerInfo>>& markersPerCamera, std::vector<ModelInfo> reconstruct_model,
                                  const std::vector<int>& rigOfModel, const std::vector<CamInfo>& cameras,
                                  const std::vector<ViewPose>& cameraPoses, std::vector<RigPoseInfo>& pose);

    // One smoothed trajectory per rig over consecutive frames (new; include/ctag_pose.h, ctag_rig_track_smooth): posesPerFrame[f] is what
    // estimateRigPose (or estimateMultiViewRigPose) returned for frame f -- a rig that is not in the list is unmeasured in that frame --
    // and covPerFrame[f][i] the covariance of posesPerFrame[f][i]: its status (CTAG_COV_OK or not) and its cov, which must be in the
    // TANGENT parametrisation, are read.  track[f][g] is frame f of rig g, for every f and every g < nRigs.  times: one per frame,
    // strictly increasing, or empty for f * opts.dt; opts: null for the defaults.  Throws std::string on error.
    void smoothRigTrack(const std::vector<std::vector<RigPoseInfo>>& posesPerFrame, const std::vector<std::vector<PoseCovInfo>>& covPerFrame,
                        int nRigs, std::vector<std::vector<TrackInfo>>& track, const std::vector<double>& times = std::vector<double>(),
                        const ctag_track_opts* opts = nullptr);

    // The live counterpart (new; include/ctag_pose.h, track filtering): startRigTracking makes a filter for nRigs rigs (every track EMPTY;
    // opts: null for the defaults) in place of any earlier one; trackRigs gives it one frame -- poses and covs as one frame's lists of
    // smoothRigTrack -- at `time` (above the last one given), or without a time at (frames given so far) * opts.dt, and returns
    // track[g] for every g < nRigs; predictRigs returns the prediction to `time` and leaves the filter as it was; stopRigTracking drops
    // the filter (the destructor does too).  They throw std::string on error.
    void startRigTracking(int nRigs, const ctag_track_filter_opts* opts = nullptr);
    // ... with the noise levels calibrateTrackNoise fitted: opts (null for the defaults) with q_rot and q_trans replaced by the fitted ones,
    // and the filter reads every covariance as noise.covScale times it (ctag_track_filter_set_cov_scale)
    void startRigTracking(int nRigs, const TrackNoiseInfo& noise, const ctag_track_filter_opts* opts = nullptr);
    void trackRigs(const std::vector<RigPoseInfo>& poses, const std::vector<PoseCovInfo>& covs, double time, std::vector<TrackInfo>& track);
    void trackRigs(const std::vector<RigPoseInfo>& poses, const std::vector<PoseCovInfo>& covs, std::vector<TrackInfo>& track);
    void predictRigs(double time, std::vector<TrackInfo>& track);
    void stopRigTracking();

    // The filter's q_rot, q_trans and covariance scale from a recorded track (new; include/ctag_pose.h, ctag_rig_track_noise_fit):
    // posesPerFrame, covPerFrame and times as smoothRigTrack takes them.  result holds one entry per rig (CTAG_NOISE_PER_RIG) or one with
    // rigID -1 (CTAG_NOISE_POOLED); opts: null for the defaults.  Throws std::string on error.
    void calibrateTrackNoise(const std::vector<std::vector<RigPoseInfo>>& posesPerFrame, const std::vector<std::vector<PoseCovInfo>>& covPerFrame,
                             int nRigs, std::vector<TrackNoiseInfo>& result, const std::vector<double>& times = std::vector<double>(),
                             const ctag_track_noise_opts* opts = nullptr);

    // The two fixed transforms between the camera's rig poses and a robot's link poses (new; include/ctag_pose.h,
    // ctag_rig_hand_eye_fit): posesPerFrame and covPerFrame as smoothRigTrack takes them, links[f] the link pose (base <- gripper) of
    // frame f; result[g] is the problem of rig g, for every g < nRigs.  opts: null for the defaults (camera on the link, no loss).
    // Throws std::string on error.
    void calibrateHandEye(const std::vector<std::vector<RigPoseInfo>>& posesPerFrame, const std::vector<std::vector<PoseCovInfo>>& covPerFrame,
                          const std::vector<LinkPose>& links, int nRigs, std::vector<HandEyeInfo>& result, const ctag_hand_eye_opts* opts = nullptr);

    // Draw the axes of the posed markers (reference: header/CylinderTag.h:33, CylinderTag.cpp:211-246): pose[i] is drawn on
    // markers[i] -- the reference pairs them by list position, after estimatePose has erased the poses without a model -- with
    // model pose[i].markerID.  The image the reference shows with imshow is kept: axisImage().  Throws std::string on error.
    void drawAxis(const ctag_host::Mat& img, std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model,
                  std::vector<PoseInfo>& pose, CamInfo camera, int axisLength = 5);
    // Same into the caller's buffer (new): img.rows rows of 3*img.cols bytes, out_step bytes apart; nothing else is written
    // and axisImage() is left as it was.
    void drawAxis(const ctag_host::Mat& img, const std::vector<MarkerInfo>& markers, const std::vector<ModelInfo>& reconstruct_model,
                  const std::vector<PoseInfo>& pose, const CamInfo& camera, int axisLength, unsigned char* out, size_t out_step);
    const AxisImage& axisImage() const { return axis_image_; }

    int featureSize() const { return featureSize_; }
    ctag_handle* handle() const { return h_; }

   private:
    void load_from_file(const std::string path);
    void load_from_set(const ctag_host::Mat1i& set_state);
    void check_dictionary(const std::vector<int>& state);
    void create(int device_id, const ctag_params* params);

    std::vector<int> state_;
    int state_rows_ = 0, state_cols_ = 0;
    int featureSize_ = 0;
    ctag_handle* h_ = nullptr;
    ctag_track_filter* filter_ = nullptr;  // startRigTracking
    int filter_rigs_ = 0;
    void track_rigs(const std::vector<RigPoseInfo>& poses, const std::vector<PoseCovInfo>& covs, const double* time, std::vector<TrackInfo>& track);
    AxisImage axis_image_;
};

#endif
