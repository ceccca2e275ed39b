// CylinderTag.cpp -- see CylinderTag.h.  Host plumbing only: every number comes from the HIP kernels behind
// the C ABI; there is no CPU implementation of the detection path here.
#include "CylinderTag.h"

#include <cstring>
#include <fstream>
#include <iostream>

#include "ctag.h"
#include "ctag_pose.h"

using ctag_host::Mat;
using ctag_host::Mat1i;
using ctag_host::Point2f;
using ctag_host::Point3f;

CylinderTag::CylinderTag(const std::string& path, int device_id, const ctag_params* params) {
    load_from_file(path);
    create(device_id, params);
}

CylinderTag::CylinderTag(const Mat1i& set_state, int feature_size, int device_id, const ctag_params* params) {
    featureSize_ = feature_size;
    load_from_set(set_state);
    create(device_id, params);
}

CylinderTag::~CylinderTag() {
    stopRigTracking();
    ctag_destroy(h_);
}

// reference: CylinderTag::load_from_file, CylinderTag.cpp:16-41
void CylinderTag::load_from_file(const std::string path) {
    std::ifstream input_file(path);
    if (!input_file.is_open()) {
        throw __FUNCTION__ + std::string(", ") + "could not open the file\n";
    }
    int marker_num = 0, marker_col = 0, feature_size = 0;
    input_file >> marker_num >> marker_col >> feature_size;
    if (marker_num < 1 || marker_col < 1) throw __FUNCTION__ + std::string(", ") + "illegal marker info\n";
    featureSize_ = feature_size;
    state_rows_ = marker_num;
    state_cols_ = marker_col;
    state_.assign((size_t)marker_num * marker_col, 0);
    for (int& i : state_) input_file >> i;
    try {
        check_dictionary(state_);
    } catch (const std::string s) {
        throw s + __FUNCTION__ + std::string(", ") + "illegal marker info\n";
    }
}

// reference: CylinderTag::load_from_set, CylinderTag.cpp:43-54
void CylinderTag::load_from_set(const Mat1i& set_state) {
    std::vector<int> v((size_t)set_state.rows * set_state.cols);
    for (int i = 0; i < set_state.rows; i++)
        for (int j = 0; j < set_state.cols; j++) v[(size_t)i * set_state.cols + j] = set_state(i, j);
    try {
        check_dictionary(v);
    } catch (const std::string s) {
        throw s + __FUNCTION__ + std::string(", ") + "illegal marker info\n";
    }
    state_ = v;
    state_rows_ = set_state.rows;
    state_cols_ = set_state.cols;
}

// reference: CylinderTag::check_dictionary, CylinderTag.cpp:56-65
void CylinderTag::check_dictionary(const std::vector<int>& input_state) {
    for (int i : input_state) {
        if (!(i >= 0 && i <= 63)) throw __FUNCTION__ + std::string(", ") + "the number in state matrix must between 0 to 63\n";
    }
}

void CylinderTag::create(int device_id, const ctag_params* params) {
    std::vector<int32_t> s(state_.begin(), state_.end());
    const int st = ctag_create_ex(s.data(), state_rows_, state_cols_, featureSize_, device_id, params, &h_);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
}

static void unflatten(const ctag_frame_result& r, std::vector<MarkerInfo>& out) {
    out.clear();
    for (int m = 0; m < r.n_markers; m++) {
        const ctag_marker_rec& M = r.markers[m];
        MarkerInfo mi;
        mi.markerID = M.marker_id;
        for (int j = 0; j < M.n_features; j++) {
            const ctag_feature_rec& F = r.features[M.first_feature + j];
            if (j < M.n_pos) mi.featurePos.push_back(F.pos);
            mi.feature_ID.push_back(F.id);
            mi.feature_ID_left.push_back(F.id_left);
            mi.feature_ID_right.push_back(F.id_right);
            std::vector<Point2f> c(8);
            for (int k = 0; k < 8; k++) c[k] = Point2f(F.corners[2 * k], F.corners[2 * k + 1]);
            mi.cornerLists.push_back(c);
            mi.feature_center.push_back(Point2f(F.center[0], F.center[1]));
            mi.edge_length.push_back(F.edge_length);
            mi.cr_left.push_back(F.cr_left);
            mi.cr_right.push_back(F.cr_right);
        }
        out.push_back(mi);
    }
}

// reference: CylinderTag::detect, CylinderTag.cpp:67-159
void CylinderTag::detect(const Mat& img, std::vector<MarkerInfo>& markers_info, int adaptiveThresh, const bool cornerSubPix,
                         int cornerSubPixDist) {
    ctag_frame_result res;
#ifdef CTAG_WITH_OPENCV
    const unsigned char* px = img.ptr<unsigned char>(0);
#else
    const unsigned char* px = img.data;
#endif
    const int st = img.channels() == 3
                       ? ctag_detect_bgr8(h_, px, img.rows, img.cols, (ptrdiff_t)img.step, adaptiveThresh, cornerSubPix ? 1 : 0, cornerSubPixDist, &res)
                       : ctag_detect_u8(h_, px, img.rows, img.cols, (ptrdiff_t)img.step, adaptiveThresh, cornerSubPix ? 1 : 0, cornerSubPixDist, &res);
    if (st == CTAG_NO_CORNER) {
        std::cout << "No corner detected!" << std::endl;  // CylinderTag.cpp:88; output left untouched
        return;
    }
    if (st == CTAG_NO_FEATURE) {
        std::cout << "No feature detected!" << std::endl;  // CylinderTag.cpp:94
        return;
    }
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    unflatten(res, markers_info);  // markers_info = markers (CylinderTag.cpp:128)
}

void CylinderTag::detectBatch(const unsigned char* frames, int n, int rows, int cols, size_t row_stride, size_t frame_stride,
                              std::vector<std::vector<MarkerInfo>>& lists, std::vector<int>& status, int adaptiveThresh,
                              const bool cornerSubPix, int cornerSubPixDist) {
    std::vector<ctag_frame_result> res((size_t)n);
    const int st = ctag_detect_batch_u8(h_, frames, n, rows, cols, (ptrdiff_t)row_stride, (ptrdiff_t)frame_stride, adaptiveThresh,
                                        cornerSubPix ? 1 : 0, cornerSubPixDist, res.data());
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    lists.resize((size_t)n);
    status.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        status[i] = res[i].status;
        if (res[i].status == CTAG_OK) unflatten(res[i], lists[i]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// pose back end (include/ctag_pose.h)
// ---------------------------------------------------------------------------------------------------------------

// reference: CylinderTag::loadModel, CylinderTag.cpp:161-190
// ctag_model -> vector<ModelInfo>
static void unpack_model(const ctag_model* m, std::vector<ModelInfo>& reconstruct_model) {
    ctag_model_view v;
    ctag_model_get_view(m, &v);
    reconstruct_model.resize((size_t)v.n_models);
    for (int i = 0; i < v.n_models; i++) {
        ModelInfo& mi = reconstruct_model[(size_t)i];
        mi.MarkerID = v.marker_id[i];
        mi.base = Point3f(v.base[3 * i], v.base[3 * i + 1], v.base[3 * i + 2]);
        mi.axis = Point3f(v.axis[3 * i], v.axis[3 * i + 1], v.axis[3 * i + 2]);
        mi.corners.resize((size_t)v.model_size * 8);
        const float* c = v.corners + (size_t)i * v.model_size * 24;
        for (int j = 0; j < v.model_size * 8; j++) mi.corners[(size_t)j] = Point3f(c[3 * j], c[3 * j + 1], c[3 * j + 2]);
    }
}

void CylinderTag::loadModel(const std::string& path, std::vector<ModelInfo>& reconstruct_model) {
    ctag_model* m = nullptr;
    if (ctag_model_load(path.c_str(), &m) != CTAG_OK) throw __FUNCTION__ + std::string(", ") + "could not open the model file\n";
    unpack_model(m, reconstruct_model);
    ctag_model_free(m);
}

// reference: CylinderTag::loadCamera, CylinderTag.cpp:192-196 (cv::FileStorage there)
void CylinderTag::loadCamera(const std::string& path, CamInfo& camera) {
    ctag_camera c;
    if (ctag_camera_load(path.c_str(), &c) != CTAG_OK) throw __FUNCTION__ + std::string(", ") + "could not read the camera file\n";
#ifdef CTAG_WITH_OPENCV
    camera.Intrinsic = cv::Mat(3, 3, CV_32F, c.K).clone();
    camera.distCoeffs = cv::Mat(c.n_dist, 1, CV_32F, c.dist).clone();
#else
    std::memcpy(camera.Intrinsic, c.K, sizeof(c.K));
    camera.distCoeffs.assign(c.dist, c.dist + c.n_dist);
#endif
}

// markers[first...] -> one flat record; returns the index of the first marker that did not fit (records hold at most
// CTAG_MAX_MARKERS markers / CTAG_MAX_FEATURES features: estimatePose walks a longer list in several records, nothing
// is dropped).  A single marker with more features than a record holds cannot come from detect() (the reference's
// father[100], corner_detector.h:143); estimatePose rejects such a list before it calls this.
static size_t flatten(const std::vector<MarkerInfo>& markers, size_t first, ctag_frame_result& r) {
    std::memset(&r, 0, sizeof(r));
    r.status = CTAG_OK;
    int nf = 0;
    size_t m = first;
    for (; m < markers.size() && r.n_markers < CTAG_MAX_MARKERS; m++) {
        const MarkerInfo& mi = markers[m];
        const int n = (int)mi.cornerLists.size();
        if (nf + n > CTAG_MAX_FEATURES) break;  // n <= CTAG_MAX_FEATURES: estimatePose validated the list
        ctag_marker_rec& M = r.markers[r.n_markers++];
        M.marker_id = mi.markerID;
        M.first_feature = nf;
        M.n_features = n;
        M.n_pos = (int)mi.featurePos.size() < n ? (int)mi.featurePos.size() : n;
        for (int j = 0; j < n; j++) {
            ctag_feature_rec& F = r.features[nf + j];
            F.pos = j < M.n_pos ? mi.featurePos[(size_t)j] : -1;
            F.id = j < (int)mi.feature_ID.size() ? mi.feature_ID[(size_t)j] : -1;
            F.id_left = j < (int)mi.feature_ID_left.size() ? mi.feature_ID_left[(size_t)j] : -1;
            F.id_right = j < (int)mi.feature_ID_right.size() ? mi.feature_ID_right[(size_t)j] : -1;
            for (int k = 0; k < 8 && k < (int)mi.cornerLists[(size_t)j].size(); k++) {
                F.corners[2 * k] = mi.cornerLists[(size_t)j][(size_t)k].x;
                F.corners[2 * k + 1] = mi.cornerLists[(size_t)j][(size_t)k].y;
            }
        }
        nf += n;
    }
    r.n_features = nf;
    return m;
}

// vector<ModelInfo> -> ctag_model (every model must hold the same number of corners, as loadModel produces); the caller frees it
static ctag_model* make_model(const std::vector<ModelInfo>& reconstruct_model, const char* who) {
    const size_t nm = reconstruct_model.size();
    const size_t per = nm ? reconstruct_model[0].corners.size() : 8;
    std::vector<int32_t> ids(nm);
    std::vector<float> base(nm * 3), axis(nm * 3), corners(nm * per * 3);
    for (size_t i = 0; i < nm; i++) {
        const ModelInfo& mi = reconstruct_model[i];
        if (mi.corners.size() != per || per % 8 != 0) throw who + std::string(", ") + "illegal model\n";
        ids[i] = mi.MarkerID;
        base[3 * i] = mi.base.x, base[3 * i + 1] = mi.base.y, base[3 * i + 2] = mi.base.z;
        axis[3 * i] = mi.axis.x, axis[3 * i + 1] = mi.axis.y, axis[3 * i + 2] = mi.axis.z;
        for (size_t j = 0; j < per; j++) {
            corners[(i * per + j) * 3] = mi.corners[j].x;
            corners[(i * per + j) * 3 + 1] = mi.corners[j].y;
            corners[(i * per + j) * 3 + 2] = mi.corners[j].z;
        }
    }
    ctag_model_view v{(int32_t)nm, (int32_t)(per / 8 ? per / 8 : 1), ids.data(), base.data(), axis.data(), corners.data()};
    ctag_model* model = nullptr;
    if (ctag_model_create(&v, &model) != CTAG_OK) throw who + std::string(", ") + "illegal model\n";
    return model;
}

// CamInfo -> ctag_camera (the matrices as float, as cameraParams.yml stores them)
static ctag_camera make_camera(const CamInfo& camera) {
    ctag_camera cam;
    std::memset(&cam, 0, sizeof(cam));
#ifdef CTAG_WITH_OPENCV
    cv::Mat Kf, Df;
    camera.Intrinsic.convertTo(Kf, CV_32F);
    camera.distCoeffs.convertTo(Df, CV_32F);
    for (int i = 0; i < 9; i++) cam.K[i] = Kf.at<float>(i / 3, i % 3);
    cam.n_dist = (int)Df.total() > 14 ? 14 : (int)Df.total();
    for (int i = 0; i < cam.n_dist; i++) cam.dist[i] = Df.ptr<float>(0)[i];
#else
    std::memcpy(cam.K, camera.Intrinsic, sizeof(cam.K));
    cam.n_dist = camera.distCoeffs.size() > 14 ? 14 : (int)camera.distCoeffs.size();
    for (int i = 0; i < cam.n_dist; i++) cam.dist[i] = camera.distCoeffs[(size_t)i];
#endif
    return cam;
}

// new: the model list from detections of the objects (include/ctag_pose.h, model reconstruction)
void CylinderTag::reconstructModel(const std::vector<std::vector<MarkerInfo>>& framesOfMarkers, const std::vector<ModelInfo>& seedModel, CamInfo camera,
                                   std::vector<ModelInfo>& outModel, double stripHeight) {
    if (framesOfMarkers.empty()) throw __FUNCTION__ + std::string(", ") + "no frames\n";
    std::vector<ctag_frame_result> recs(framesOfMarkers.size());
    for (size_t f = 0; f < framesOfMarkers.size(); f++) {
        for (const MarkerInfo& mi : framesOfMarkers[f])
            if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw __FUNCTION__ + std::string(", ") + "a marker with more than 100 features\n";
        if (flatten(framesOfMarkers[f], 0, recs[f]) != framesOfMarkers[f].size())
            throw __FUNCTION__ + std::string(", ") + "a frame with more markers or features than a detection record holds\n";
        if (recs[f].n_markers == 0) recs[f].status = CTAG_NO_FEATURE;  // detect() left the list empty
    }
    ctag_model* seed = make_model(seedModel, __FUNCTION__);
    const ctag_camera cam = make_camera(camera);
    ctag_model_fit_opts opts;
    ctag_model_fit_opts_default(&opts);
    opts.strip_height = stripHeight;
    std::vector<ctag_model_fit_stat> stats(seedModel.size() + 1);
    ctag_model* fitted = nullptr;
    const int st = ctag_model_fit(h_, recs.data(), (int)recs.size(), seed, &cam, &opts, &fitted, stats.data());
    ctag_model_free(seed);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    unpack_model(fitted, outModel);
    ctag_model_free(fitted);
}

// new: the models of every rig in one frame (include/ctag_pose.h, rig assembly)
void CylinderTag::assembleRigModel(const std::vector<std::vector<MarkerInfo>>& framesOfMarkers, const std::vector<ModelInfo>& model,
                                   const std::vector<int>& rigOfModel, CamInfo camera, std::vector<ModelInfo>& outModel, std::vector<int>& placedRigOfModel) {
    if (framesOfMarkers.empty()) throw __FUNCTION__ + std::string(", ") + "no frames\n";
    if (rigOfModel.size() != model.size()) throw __FUNCTION__ + std::string(", ") + "one rig entry per model\n";
    int n_rigs = 1;
    for (int g : rigOfModel) n_rigs = g + 1 > n_rigs ? g + 1 : n_rigs;
    std::vector<ctag_frame_result> recs(framesOfMarkers.size());
    for (size_t f = 0; f < framesOfMarkers.size(); f++) {
        for (const MarkerInfo& mi : framesOfMarkers[f])
            if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw __FUNCTION__ + std::string(", ") + "a marker with more than 100 features\n";
        if (flatten(framesOfMarkers[f], 0, recs[f]) != framesOfMarkers[f].size())
            throw __FUNCTION__ + std::string(", ") + "a frame with more markers or features than a detection record holds\n";
        if (recs[f].n_markers == 0) recs[f].status = CTAG_NO_FEATURE;  // detect() left the list empty
    }
    ctag_model* in = make_model(model, __FUNCTION__);
    ctag_rigs* rigs = nullptr;
    int st = ctag_rigs_create(in, rigOfModel.data(), n_rigs, &rigs);
    if (st != CTAG_OK) {
        ctag_model_free(in);
        throw __FUNCTION__ + std::string(", ") + "illegal rig set\n";
    }
    const ctag_camera cam = make_camera(camera);
    std::vector<ctag_rig_fit_stat> rig_stats((size_t)n_rigs);
    std::vector<ctag_rig_fit_model_stat> model_stats(model.size() + 1);
    ctag_model* assembled = nullptr;
    st = ctag_rig_fit(h_, recs.data(), (int)recs.size(), in, rigs, &cam, nullptr, &assembled, rig_stats.data(), model_stats.data());
    ctag_rigs_free(rigs);
    ctag_model_free(in);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    unpack_model(assembled, outModel);
    ctag_model_free(assembled);
    placedRigOfModel.assign(rigOfModel.begin(), rigOfModel.end());
    for (size_t m = 0; m < model.size(); m++)
        if (model_stats[m].status != CTAG_POSE_OK) placedRigOfModel[m] = -1;
}

// new: the poses of the cameras of a set (include/ctag_pose.h, camera set fit)
bool CylinderTag::calibrateCameraSet(const std::vector<std::vector<std::vector<MarkerInfo>>>& markersPerCamera, const std::vector<ModelInfo>& model,
                                     const std::vector<int>& rigOfModel, const std::vector<CamInfo>& cameras, std::vector<ViewPose>& cameraPoses,
                                     std::vector<int>& placed) {
    const size_t nc = cameras.size();
    if (nc < 2 || nc > (size_t)CTAG_MV_MAX_CAMERAS) throw __FUNCTION__ + std::string(", ") + "2 to 8 cameras\n";
    if (markersPerCamera.size() != nc) throw __FUNCTION__ + std::string(", ") + "one list of instants per camera\n";
    const size_t nf = markersPerCamera[0].size();
    if (nf == 0) throw __FUNCTION__ + std::string(", ") + "no instants\n";
    if (rigOfModel.size() != model.size()) throw __FUNCTION__ + std::string(", ") + "one rig entry per model\n";
    int n_rigs = 1;
    for (int g : rigOfModel) n_rigs = g + 1 > n_rigs ? g + 1 : n_rigs;
    std::vector<ctag_frame_result> recs(nc * nf);  // camera-major
    std::vector<ctag_camera> cams(nc);
    for (size_t c = 0; c < nc; c++) {
        if (markersPerCamera[c].size() != nf) throw __FUNCTION__ + std::string(", ") + "every camera has the same instants\n";
        cams[c] = make_camera(cameras[c]);
        for (size_t f = 0; f < nf; f++) {
            const std::vector<MarkerInfo>& list = markersPerCamera[c][f];
            ctag_frame_result& r = recs[c * nf + f];
            for (const MarkerInfo& mi : list)
                if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw __FUNCTION__ + std::string(", ") + "a marker with more than 100 features\n";
            if (flatten(list, 0, r) != list.size()) throw __FUNCTION__ + std::string(", ") + "an instant with more markers or features than a detection record holds\n";
            if (r.n_markers == 0) r.status = CTAG_NO_FEATURE;  // detect() left the list empty
        }
    }
    ctag_model* in = make_model(model, __FUNCTION__);
    ctag_rigs* rigs = nullptr;
    int st = ctag_rigs_create(in, rigOfModel.data(), n_rigs, &rigs);
    if (st != CTAG_OK) {
        ctag_model_free(in);
        throw __FUNCTION__ + std::string(", ") + "illegal rig set\n";
    }
    ctag_camera_fit_stat stat;
    std::vector<ctag_camera_fit_cam_stat> cam_stats(nc);
    ctag_camera_set* set = nullptr;
    st = ctag_camera_fit(h_, recs.data(), (int)nc, (int)nf, in, rigs, cams.data(), nullptr, &set, &stat, cam_stats.data());
    ctag_rigs_free(rigs);
    ctag_model_free(in);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    if (set) ctag_camera_set_free(set);
    cameraPoses.assign(nc, ViewPose());
    placed.assign(nc, 0);
    for (size_t c = 0; c < nc; c++) {
        placed[c] = cam_stats[c].status == CTAG_POSE_OK ? 1 : 0;
#ifdef CTAG_WITH_OPENCV
        cameraPoses[c].rvec = cv::Mat(3, 1, CV_64F);
        cameraPoses[c].tvec = cv::Mat(3, 1, CV_64F);
        double *pr = cameraPoses[c].rvec.ptr<double>(0), *pt = cameraPoses[c].tvec.ptr<double>(0);
#else
        double *pr = cameraPoses[c].rvec, *pt = cameraPoses[c].tvec;
#endif
        for (int i = 0; i < 3; i++) {
            pr[i] = cam_stats[c].pose.rvec[i];
            pt[i] = cam_stats[c].pose.tvec[i];
        }
    }
    return stat.n_unplaced == 0 && stat.status == CTAG_POSE_OK;
}

// new: the camera's intrinsics from views of known rigs (include/ctag_pose.h, intrinsics fit)
bool CylinderTag::calibrateCamera(const std::vector<std::vector<MarkerInfo>>& markersPerFrame, const std::vector<ModelInfo>& model, const std::vector<int>& rigOfModel,
                                  CamInfo seed, CamInfo& camera, std::vector<double>* sigma, unsigned freeMask, bool tieFocal) {
    if (markersPerFrame.empty()) throw __FUNCTION__ + std::string(", ") + "no frames\n";
    std::vector<int> rig(rigOfModel);
    if (rig.empty())
        for (size_t m = 0; m < model.size(); m++) rig.push_back((int)m);
    if (rig.size() != model.size()) throw __FUNCTION__ + std::string(", ") + "one rig entry per model\n";
    int n_rigs = 1;
    for (int g : rig) n_rigs = g + 1 > n_rigs ? g + 1 : n_rigs;
    std::vector<ctag_frame_result> recs(markersPerFrame.size());
    for (size_t f = 0; f < markersPerFrame.size(); f++) {
        for (const MarkerInfo& mi : markersPerFrame[f])
            if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw __FUNCTION__ + std::string(", ") + "a marker with more than 100 features\n";
        if (flatten(markersPerFrame[f], 0, recs[f]) != markersPerFrame[f].size())
            throw __FUNCTION__ + std::string(", ") + "a frame with more markers or features than a detection record holds\n";
        if (recs[f].n_markers == 0) recs[f].status = CTAG_NO_FEATURE;  // detect() left the list empty
    }
    ctag_model* in = make_model(model, __FUNCTION__);
    ctag_rigs* rigs = nullptr;
    int st = ctag_rigs_create(in, rig.data(), n_rigs, &rigs);
    if (st != CTAG_OK) {
        ctag_model_free(in);
        throw __FUNCTION__ + std::string(", ") + "illegal rig set\n";
    }
    const ctag_camera cam0 = make_camera(seed);
    ctag_intrinsics_fit_opts opts;
    ctag_intrinsics_fit_opts_default(&opts);
    opts.free_mask = freeMask;
    opts.tie_focal = tieFocal ? 1 : 0;
    ctag_camera cam;
    ctag_intrinsics_fit_stat stat;
    st = ctag_intrinsics_fit(h_, recs.data(), (int)recs.size(), in, rigs, &cam0, &opts, &cam, &stat, nullptr);
    ctag_rigs_free(rigs);
    ctag_model_free(in);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    camera = seed;
#ifdef CTAG_WITH_OPENCV
    camera.Intrinsic = cv::Mat(3, 3, CV_32F, cam.K).clone();  // float, as cameraParams.yml stores them
    if (cam.n_dist > 0) camera.distCoeffs = cv::Mat(cam.n_dist, 1, CV_32F, cam.dist).clone();
#else
    std::memcpy(camera.Intrinsic, cam.K, sizeof(cam.K));
    for (int i = 0; i < cam.n_dist; i++) camera.distCoeffs[(size_t)i] = cam.dist[i];
#endif
    if (sigma) sigma->assign(stat.sigma, stat.sigma + CTAG_INTR_PARAMS);
    return stat.status == CTAG_POSE_OK;
}

void CylinderTag::saveModel(const std::string& path, const std::vector<ModelInfo>& model) {
    ctag_model* m = make_model(model, __FUNCTION__);
    const int st = ctag_model_save(m, path.c_str());
    ctag_model_free(m);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + "could not write the model file\n";
}

// reference: CylinderTag::estimatePose, CylinderTag.cpp:198-209 (+ PoseEstimator::PnPSolver / PoseBA)
void CylinderTag::estimatePose(const Mat& img, std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, CamInfo camera,
                               std::vector<PoseInfo>& pose, bool useDensePoseRefine) {
    (void)img;
    (void)useDensePoseRefine;
    pose.clear();
    if (markers.empty()) return;
    for (const MarkerInfo& mi : markers)  // checked before anything is allocated: flatten() cannot fail afterwards
        if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw std::string("estimatePose, a marker with more than 100 features\n");
    ctag_model* model = make_model(reconstruct_model, __FUNCTION__);
    const ctag_camera cam = make_camera(camera);
    std::vector<ctag_pose_rec> rec;
    for (size_t first = 0; first < markers.size();) {  // any number of markers: one record (<= 100 markers / features) at a time
        ctag_frame_result res;
        const size_t next = flatten(markers, first, res);
        const size_t at = rec.size();
        rec.resize(at + (size_t)res.n_markers);
        const int st = ctag_estimate_pose(h_, &res, model, &cam, rec.data() + at);
        if (st != CTAG_OK) {
            ctag_model_free(model);
            throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
        }
        first = next;
    }
    ctag_model_free(model);
    for (const ctag_pose_rec& p : rec) {
        if (p.status == CTAG_POSE_NO_MODEL) continue;  // pose.erase(remove_if(markerID == -1)), CylinderTag.cpp:206-208
        if (p.status != CTAG_POSE_OK)  // cv::solvePnP throws on < 4 points; an out-of-model position is UB in the reference
            throw __FUNCTION__ + std::string(", ") + "marker without a usable point set\n";
        PoseInfo pi;
        pi.markerID = p.model_index;
#ifdef CTAG_WITH_OPENCV
        pi.rvec = (cv::Mat_<double>(3, 1) << p.rvec[0], p.rvec[1], p.rvec[2]);
        pi.tvec = (cv::Mat_<double>(3, 1) << p.tvec[0], p.tvec[1], p.tvec[2]);
#else
        for (int i = 0; i < 3; i++) {
            pi.rvec[i] = p.rvec[i];
            pi.tvec[i] = p.tvec[i];
        }
#endif
        pose.push_back(pi);
    }
}

void CylinderTag::estimatePoseCovariance(std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, CamInfo camera,
                                         std::vector<PoseCovInfo>& covariance, bool tangent, double sigmaPx, double outlierK) {
    covariance.clear();
    if (markers.empty()) return;
    for (const MarkerInfo& mi : markers)
        if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw std::string("estimatePoseCovariance, a marker with more than 100 features\n");
    ctag_model* model = make_model(reconstruct_model, __FUNCTION__);
    const ctag_camera cam = make_camera(camera);
    ctag_cov_opts opts;
    ctag_cov_opts_default(&opts);
    opts.param = tangent ? CTAG_COV_PARAM_TANGENT : CTAG_COV_PARAM_RVEC;
    opts.sigma_px = sigmaPx;
    opts.outlier_k = outlierK;
    std::vector<ctag_pose_rec> rec;
    std::vector<ctag_pose_cov_rec> cov;
    for (size_t first = 0; first < markers.size();) {  // one record (<= 100 markers / features) at a time, as estimatePose
        ctag_frame_result res;
        const size_t next = flatten(markers, first, res);
        const size_t at = rec.size();
        rec.resize(at + (size_t)res.n_markers);
        cov.resize(at + (size_t)res.n_markers);
        int st = ctag_estimate_pose(h_, &res, model, &cam, rec.data() + at);
        if (st == CTAG_OK) st = ctag_estimate_pose_cov(h_, &res, model, &cam, rec.data() + at, &opts, cov.data() + at);
        if (st != CTAG_OK) {
            ctag_model_free(model);
            throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
        }
        first = next;
    }
    ctag_model_free(model);
    for (size_t i = 0; i < rec.size(); i++) {
        if (rec[i].status == CTAG_POSE_NO_MODEL) continue;  // erased, as in estimatePose
        if (rec[i].status != CTAG_POSE_OK) throw __FUNCTION__ + std::string(", ") + "marker without a usable point set\n";
        const ctag_pose_cov_rec& c = cov[i];
        PoseCovInfo ci;
        ci.markerID = rec[i].model_index;
        ci.status = c.status;
        ci.nPoints = c.n_points;
        ci.dof = c.dof;
        ci.worstPoint = c.worst_point;
        ci.nOutliers = c.n_outliers;
        ci.cost = c.cost;
        ci.sigma2Hat = c.sigma2_hat;
        ci.sigma2Used = c.sigma2_used;
        ci.maxResidualPx = c.max_residual_px;
        ci.minPivot = c.min_pivot;
        for (int k = 0; k < 36; k++) ci.cov[k] = c.cov[k];
        covariance.push_back(ci);
    }
}

void CylinderTag::estimatePoseRobust(std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, CamInfo camera,
                                     std::vector<RobustPoseInfo>& robust, bool cauchy, double scalePx, int maxIterations) {
    robust.clear();
    if (markers.empty()) return;
    for (const MarkerInfo& mi : markers)
        if (mi.cornerLists.size() > (size_t)CTAG_MAX_FEATURES) throw std::string("estimatePoseRobust, a marker with more than 100 features\n");
    ctag_model* model = make_model(reconstruct_model, __FUNCTION__);
    const ctag_camera cam = make_camera(camera);
    ctag_robust_opts opts;
    ctag_robust_opts_default(&opts);
    opts.loss = cauchy ? CTAG_LOSS_CAUCHY : CTAG_LOSS_HUBER;
    opts.scale_px = scalePx;
    opts.max_iterations = maxIterations;
    std::vector<ctag_pose_rec> rec;
    std::vector<ctag_robust_pose_rec> rob;
    for (size_t first = 0; first < markers.size();) {  // one record (<= 100 markers / features) at a time, as estimatePose
        ctag_frame_result res;
        const size_t next = flatten(markers, first, res);
        const size_t at = rec.size();
        rec.resize(at + (size_t)res.n_markers);
        rob.resize(at + (size_t)res.n_markers);
        int st = ctag_estimate_pose(h_, &res, model, &cam, rec.data() + at);
        if (st == CTAG_OK) st = ctag_estimate_pose_robust(h_, &res, model, &cam, rec.data() + at, &opts, rob.data() + at);
        if (st != CTAG_OK) {
            ctag_model_free(model);
            throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
        }
        first = next;
    }
    ctag_model_free(model);
    for (size_t i = 0; i < rec.size(); i++) {
        if (rec[i].status == CTAG_POSE_NO_MODEL) continue;  // erased, as in estimatePose
        if (rec[i].status != CTAG_POSE_OK) throw __FUNCTION__ + std::string(", ") + "marker without a usable point set\n";
        const ctag_robust_pose_rec& r = rob[i];
        RobustPoseInfo ri;
        ri.markerID = rec[i].model_index;
        ri.status = r.status;
        ri.nPoints = r.n_points;
        ri.nInliers = r.n_inliers;
        ri.iterations = r.iterations;
        ri.loss = r.loss;
        ri.worstPoint = r.worst_point;
        ri.inlier.resize((size_t)r.n_points);
        for (int k = 0; k < r.n_points; k++) ri.inlier[(size_t)k] = ((r.inlier_mask[k >> 5] >> (k & 31)) & 1u) != 0;
        ri.scalePx = r.scale_px;
        ri.sigmaHat = r.sigma_hat;
        ri.costLs0 = r.cost_ls0;
        ri.costLs = r.cost_ls;
        ri.cost0 = r.cost0;
        ri.cost = r.cost;
        ri.maxResidualPx = r.max_residual_px;
        for (int k = 0; k < 3; k++) {
            ri.rvec[k] = r.rvec[k];
            ri.tvec[k] = r.tvec[k];
        }
        robust.push_back(ri);
    }
}

void CylinderTag::estimateRigPose(std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, const std::vector<int>& rigOfModel,
                                  CamInfo camera, std::vector<RigPoseInfo>& pose) {
    pose.clear();
    if (rigOfModel.size() != reconstruct_model.size()) throw __FUNCTION__ + std::string(", ") + "one rig entry per model\n";
    int n_rigs = 0;
    for (int g : rigOfModel) n_rigs = g + 1 > n_rigs ? g + 1 : n_rigs;
    if (markers.empty() || n_rigs == 0) return;
    if (markers.size() > (size_t)CTAG_MAX_MARKERS) throw __FUNCTION__ + std::string(", ") + "more than 100 markers\n";
    ctag_frame_result res;
    if (flatten(markers, 0, res) != markers.size()) throw __FUNCTION__ + std::string(", ") + "more than 100 features\n";
    ctag_model* model = make_model(reconstruct_model, __FUNCTION__);
    ctag_rigs* rigs = nullptr;
    int st = ctag_rigs_create(model, rigOfModel.data(), n_rigs, &rigs);
    std::vector<ctag_rig_pose_rec> rec((size_t)n_rigs);
    const ctag_camera cam = make_camera(camera);
    if (st == CTAG_OK) st = ctag_estimate_rig_pose(h_, &res, model, rigs, &cam, rec.data());
    ctag_rigs_free(rigs);
    ctag_model_free(model);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    for (const ctag_rig_pose_rec& p : rec) {
        if (p.status == CTAG_POSE_NOT_SEEN) continue;  // erased, as estimatePose erases markers without a model
        if (p.status != CTAG_POSE_OK) throw __FUNCTION__ + std::string(", ") + "rig without a usable point set\n";
        RigPoseInfo ri;
        ri.rigID = p.rig;
#ifdef CTAG_WITH_OPENCV
        ri.rvec = (cv::Mat_<double>(3, 1) << p.rvec[0], p.rvec[1], p.rvec[2]);
        ri.tvec = (cv::Mat_<double>(3, 1) << p.tvec[0], p.tvec[1], p.tvec[2]);
#else
        for (int i = 0; i < 3; i++) {
            ri.rvec[i] = p.rvec[i];
            ri.tvec[i] = p.tvec[i];
        }
#endif
        for (int k = 0; k < CTAG_MAX_MARKERS; k++)
            if ((p.member_mask[k >> 5] >> (k & 31)) & 1u) ri.members.push_back(k);
        pose.push_back(ri);
    }
}

void CylinderTag::estimateMultiViewRigPose(const std::vector<std::vector<MarkerInfo>>& markersPerCamera, std::vector<ModelInfo> reconstruct_model,
                                           const std::vector<int>& rigOfModel, const std::vector<CamInfo>& cameras,
                                           const std::vector<ViewPose>& cameraPoses, std::vector<RigPoseInfo>& pose) {
    pose.clear();
    const size_t nc = cameras.size();
    if (nc < 1 || nc > (size_t)CTAG_MV_MAX_CAMERAS) throw __FUNCTION__ + std::string(", ") + "1 to 8 cameras\n";
    if (markersPerCamera.size() != nc || cameraPoses.size() != nc) throw __FUNCTION__ + std::string(", ") + "one marker list and one pose per camera\n";
    if (rigOfModel.size() != reconstruct_model.size()) throw __FUNCTION__ + std::string(", ") + "one rig entry per model\n";
    int n_rigs = 0;
    for (int g : rigOfModel) n_rigs = g + 1 > n_rigs ? g + 1 : n_rigs;
    if (n_rigs == 0) return;
    std::vector<ctag_frame_result> res(nc);
    std::vector<ctag_camera> cams(nc);
    std::vector<ctag_camera_pose> cps(nc);
    for (size_t c = 0; c < nc; c++) {
        if (markersPerCamera[c].size() > (size_t)CTAG_MAX_MARKERS) throw __FUNCTION__ + std::string(", ") + "more than 100 markers\n";
        if (flatten(markersPerCamera[c], 0, res[c]) != markersPerCamera[c].size()) throw __FUNCTION__ + std::string(", ") + "more than 100 features\n";
        cams[c] = make_camera(cameras[c]);
#ifdef CTAG_WITH_OPENCV
        cv::Mat r64, t64;
        cameraPoses[c].rvec.convertTo(r64, CV_64F);
        cameraPoses[c].tvec.convertTo(t64, CV_64F);
        if (r64.total() != 3 || t64.total() != 3) throw __FUNCTION__ + std::string(", ") + "a camera pose is two 3-vectors\n";
        const double *pr = r64.ptr<double>(0), *pt = t64.ptr<double>(0);
#else
        const double *pr = cameraPoses[c].rvec, *pt = cameraPoses[c].tvec;
#endif
        for (int i = 0; i < 3; i++) {
            cps[c].rvec[i] = pr[i];
            cps[c].tvec[i] = pt[i];
        }
    }
    ctag_camera_set* set = nullptr;
    int st = ctag_camera_set_create(cams.data(), cps.data(), (int)nc, &set);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    ctag_model* model = nullptr;
    try {
        model = make_model(reconstruct_model, __FUNCTION__);
    } catch (...) {
        ctag_camera_set_free(set);
        throw;
    }
    ctag_rigs* rigs = nullptr;
    st = ctag_rigs_create(model, rigOfModel.data(), n_rigs, &rigs);
    std::vector<ctag_mv_pose_rec> rec((size_t)n_rigs);
    if (st == CTAG_OK) st = ctag_estimate_mv_rig_pose(h_, res.data(), model, rigs, set, rec.data());
    ctag_rigs_free(rigs);
    ctag_model_free(model);
    ctag_camera_set_free(set);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    for (const ctag_mv_pose_rec& p : rec) {
        if (p.status == CTAG_POSE_NOT_SEEN) continue;  // erased, as estimateRigPose erases rigs without a member
        if (p.status != CTAG_POSE_OK) throw __FUNCTION__ + std::string(", ") + "rig without a usable point set\n";
        RigPoseInfo ri;
        ri.rigID = p.rig;
#ifdef CTAG_WITH_OPENCV
        ri.rvec = (cv::Mat_<double>(3, 1) << p.rvec[0], p.rvec[1], p.rvec[2]);
        ri.tvec = (cv::Mat_<double>(3, 1) << p.tvec[0], p.tvec[1], p.tvec[2]);
#else
        for (int i = 0; i < 3; i++) {
            ri.rvec[i] = p.rvec[i];
            ri.tvec[i] = p.tvec[i];
        }
#endif
        for (int c = 0; c < (int)nc; c++)
            for (int k = 0; k < CTAG_MAX_MARKERS; k++)
                if ((p.member_mask[c][k >> 5] >> (k & 31)) & 1u) ri.viewMembers.emplace_back(c, k);
        pose.push_back(ri);
    }
}

// the per-frame lists of estimateRigPose and their covariances as the n_frames x nRigs records of the batch calls: a rig that is not in a
// frame's list is CTAG_POSE_NOT_SEEN there.  `who` names the caller in what is thrown; times: the caller's, checked where smoothRigTrack
// has always checked them, or null.
static void rig_records(const std::string& who, const std::vector<std::vector<RigPoseInfo>>& posesPerFrame,
                        const std::vector<std::vector<PoseCovInfo>>& covPerFrame, int nRigs, unsigned long long max_items,
                        const std::vector<double>* times, std::vector<ctag_rig_pose_rec>& rec, std::vector<ctag_pose_cov_rec>& cov) {
    const size_t n_frames = posesPerFrame.size();
    if (n_frames == 0) throw who + ", no frames\n";
    if (covPerFrame.size() != n_frames) throw who + ", one covariance list per frame\n";
    if (nRigs < 1 || (unsigned long long)n_frames * (unsigned long long)nRigs > max_items) throw who + ", frames x rigs outside 1 .. 65536\n";
    if (times && !times->empty() && times->size() != n_frames) throw who + ", one time per frame\n";
    const size_t n = n_frames * (size_t)nRigs;
    rec.resize(n);
    cov.resize(n);
    std::memset(rec.data(), 0, sizeof(ctag_rig_pose_rec) * n);
    std::memset(cov.data(), 0, sizeof(ctag_pose_cov_rec) * n);
    for (size_t f = 0; f < n_frames; f++) {
        for (int g = 0; g < nRigs; g++) {
            rec[f * nRigs + g].status = CTAG_POSE_NOT_SEEN;
            rec[f * nRigs + g].rig = g;
            rec[f * nRigs + g].frame = (int32_t)f;
            cov[f * nRigs + g].status = CTAG_COV_NO_POSE;
        }
        if (covPerFrame[f].size() != posesPerFrame[f].size()) throw who + ", one covariance per pose\n";
        for (size_t i = 0; i < posesPerFrame[f].size(); i++) {
            const RigPoseInfo& p = posesPerFrame[f][i];
            if (p.rigID < 0 || p.rigID >= nRigs) throw who + ", a rig outside 0 .. nRigs - 1\n";
            ctag_rig_pose_rec& r = rec[f * nRigs + p.rigID];
            if (r.status == CTAG_POSE_OK) throw who + ", a rig twice in one frame\n";
            r.status = CTAG_POSE_OK;
#ifdef CTAG_WITH_OPENCV
            const double *pr = p.rvec.ptr<double>(0), *pt = p.tvec.ptr<double>(0);
#else
            const double *pr = p.rvec, *pt = p.tvec;
#endif
            for (int k = 0; k < 3; k++) {
                r.rvec[k] = pr[k];
                r.tvec[k] = pt[k];
            }
            ctag_pose_cov_rec& c = cov[f * nRigs + p.rigID];
            c.status = covPerFrame[f][i].status;
            c.param = CTAG_COV_PARAM_TANGENT;
            for (int k = 0; k < 36; k++) c.cov[k] = covPerFrame[f][i].cov[k];
        }
    }
}

// the smoother and the hand-eye fit read n_rigs of the rig set and nothing else: a set of nRigs one-model rigs over a model made for it
struct CountRigs {
    ctag_model* model = nullptr;
    ctag_rigs* rigs = nullptr;
    int status = CTAG_OK;
    explicit CountRigs(int nRigs) {
        std::vector<int32_t> ids(nRigs), rig_of_model(nRigs);
        std::vector<float> zeros3((size_t)nRigs * 3, 0.f), corners((size_t)nRigs * 24, 0.f);
        for (int g = 0; g < nRigs; g++) ids[g] = rig_of_model[g] = g;
        ctag_model_view mv;
        mv.n_models = nRigs;
        mv.model_size = 1;
        mv.marker_id = ids.data();
        mv.base = zeros3.data();
        mv.axis = zeros3.data();
        mv.corners = corners.data();
        status = ctag_model_create(&mv, &model);
        if (status == CTAG_OK) status = ctag_rigs_create(model, rig_of_model.data(), nRigs, &rigs);
    }
    ~CountRigs() {
        if (rigs) ctag_rigs_free(rigs);
        if (model) ctag_model_free(model);
    }
    CountRigs(const CountRigs&) = delete;
    CountRigs& operator=(const CountRigs&) = delete;
};

// a track record of either the smoother or the filter as the class returns it
static void track_info(const ctag_track_rec& t, TrackInfo& ti) {
    ti.rigID = t.rig;
    ti.status = t.status;
    ti.measured = (t.flags & CTAG_TRACK_FLAG_MEASURED) != 0;
    ti.downweighted = (t.flags & CTAG_TRACK_FLAG_DOWNWEIGHTED) != 0;
    ti.gated = (t.flags & CTAG_TRACK_FLAG_GATED) != 0;
    ti.started = (t.flags & CTAG_TRACK_FLAG_STARTED) != 0;
    for (int k = 0; k < 3; k++) {
        ti.rvec[k] = t.rvec[k];
        ti.tvec[k] = t.tvec[k];
        ti.w[k] = t.w[k];
        ti.v[k] = t.v[k];
    }
    for (int k = 0; k < 36; k++) ti.cov[k] = t.cov[k];
    for (int k = 0; k < 6; k++) ti.velSigma[k] = t.vel_sigma[k];
    ti.mahalanobis2 = t.mahalanobis2;
    ti.weight = t.weight;
}

void CylinderTag::smoothRigTrack(const std::vector<std::vector<RigPoseInfo>>& posesPerFrame, const std::vector<std::vector<PoseCovInfo>>& covPerFrame,
                                 int nRigs, std::vector<std::vector<TrackInfo>>& track, const std::vector<double>& times, const ctag_track_opts* opts) {
    track.clear();
    std::vector<ctag_rig_pose_rec> rec;
    std::vector<ctag_pose_cov_rec> cov;
    rig_records("smoothRigTrack", posesPerFrame, covPerFrame, nRigs, CTAG_TRACK_MAX_ITEMS, &times, rec, cov);
    const size_t n_frames = posesPerFrame.size(), n = rec.size();
    CountRigs set(nRigs);
    int st = set.status;
    std::vector<ctag_track_rec> out(n);
    std::vector<ctag_track_stat> stat((size_t)nRigs);
    if (st == CTAG_OK)
        st = ctag_rig_track_smooth(h_, set.rigs, rec.data(), cov.data(), (int)n_frames, times.empty() ? nullptr : times.data(), opts, out.data(), stat.data());
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    track.assign(n_frames, std::vector<TrackInfo>((size_t)nRigs));
    for (size_t f = 0; f < n_frames; f++)
        for (int g = 0; g < nRigs; g++) track_info(out[f * nRigs + g], track[f][g]);
}

void CylinderTag::stopRigTracking() {
    if (filter_) ctag_track_filter_free(filter_);
    filter_ = nullptr;
    filter_rigs_ = 0;
}

void CylinderTag::startRigTracking(int nRigs, const ctag_track_filter_opts* opts) {
    stopRigTracking();
    if (nRigs < 1 || nRigs > CTAG_TRACK_MAX_ITEMS) throw std::string("startRigTracking, rigs outside 1 .. 65536\n");
    CountRigs set(nRigs);
    int st = set.status;
    if (st == CTAG_OK) st = ctag_track_filter_create(h_, set.rigs, opts, &filter_);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    filter_rigs_ = nRigs;
}

void CylinderTag::startRigTracking(int nRigs, const TrackNoiseInfo& noise, const ctag_track_filter_opts* opts) {
    ctag_track_filter_opts o;
    ctag_track_filter_opts_default(&o);
    if (opts) o = *opts;
    o.q_rot = noise.qRot;
    o.q_trans = noise.qTrans;
    startRigTracking(nRigs, &o);
    const int st = ctag_track_filter_set_cov_scale(filter_, noise.covScale);
    if (st != CTAG_OK) {
        stopRigTracking();
        throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    }
}

void CylinderTag::calibrateTrackNoise(const std::vector<std::vector<RigPoseInfo>>& posesPerFrame, const std::vector<std::vector<PoseCovInfo>>& covPerFrame,
                                      int nRigs, std::vector<TrackNoiseInfo>& result, const std::vector<double>& times, const ctag_track_noise_opts* opts) {
    result.clear();
    std::vector<ctag_rig_pose_rec> rec;
    std::vector<ctag_pose_cov_rec> cov;
    rig_records("calibrateTrackNoise", posesPerFrame, covPerFrame, nRigs, CTAG_TRACK_MAX_ITEMS, &times, rec, cov);
    const size_t n_frames = posesPerFrame.size();
    CountRigs set(nRigs);
    int st = set.status;
    const size_t n_search = opts && opts->mode == CTAG_NOISE_POOLED ? 1 : (size_t)nRigs;
    std::vector<ctag_track_noise_rec> out(n_search);
    if (st == CTAG_OK)
        st = ctag_rig_track_noise_fit(h_, set.rigs, rec.data(), cov.data(), (int)n_frames, times.empty() ? nullptr : times.data(), opts, out.data(), nullptr);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    result.resize(n_search);
    for (size_t q = 0; q < n_search; q++) {
        const ctag_track_noise_rec& r = out[q];
        TrackNoiseInfo& ni = result[q];
        ni.rigID = r.rig;
        ni.status = r.status;
        ni.nTerms = r.n_terms;
        ni.nFree = r.n_free;
        ni.rounds = r.rounds;
        ni.flags = r.flags;
        ni.qRot = r.q_rot;
        ni.qTrans = r.q_trans;
        ni.covScale = r.cov_scale;
        for (int k = 0; k < 3; k++) ni.log2Sigma[k] = r.log2_sigma[k];
        ni.score = r.score;
        ni.scoreStart = r.score_start;
        ni.meanM2 = r.mean_m2;
    }
}

void CylinderTag::track_rigs(const std::vector<RigPoseInfo>& poses, const std::vector<PoseCovInfo>& covs, const double* time, std::vector<TrackInfo>& track) {
    track.clear();
    if (!filter_) throw std::string("trackRigs, startRigTracking first\n");
    std::vector<ctag_rig_pose_rec> rec;
    std::vector<ctag_pose_cov_rec> cov;
    rig_records("trackRigs", {poses}, {covs}, filter_rigs_, CTAG_TRACK_MAX_ITEMS, nullptr, rec, cov);
    std::vector<ctag_track_rec> out(rec.size());
    const int st = ctag_rig_track_filter(filter_, rec.data(), cov.data(), 1, time, out.data());
    if (st != CTAG_OK) throw std::string("trackRigs, ") + ctag_strerror(st) + "\n";
    track.resize(out.size());
    for (size_t g = 0; g < out.size(); g++) track_info(out[g], track[g]);
}

void CylinderTag::trackRigs(const std::vector<RigPoseInfo>& poses, const std::vector<PoseCovInfo>& covs, double time, std::vector<TrackInfo>& track) {
    track_rigs(poses, covs, &time, track);
}

void CylinderTag::trackRigs(const std::vector<RigPoseInfo>& poses, const std::vector<PoseCovInfo>& covs, std::vector<TrackInfo>& track) {
    track_rigs(poses, covs, nullptr, track);
}

void CylinderTag::predictRigs(double time, std::vector<TrackInfo>& track) {
    track.clear();
    if (!filter_) throw std::string("predictRigs, startRigTracking first\n");
    std::vector<ctag_track_rec> out((size_t)filter_rigs_);
    const int st = ctag_track_filter_predict(filter_, time, out.data());
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    track.resize(out.size());
    for (size_t g = 0; g < out.size(); g++) track_info(out[g], track[g]);
}

void CylinderTag::calibrateHandEye(const std::vector<std::vector<RigPoseInfo>>& posesPerFrame, const std::vector<std::vector<PoseCovInfo>>& covPerFrame,
                                   const std::vector<LinkPose>& links, int nRigs, std::vector<HandEyeInfo>& result, const ctag_hand_eye_opts* opts) {
    result.clear();
    std::vector<ctag_rig_pose_rec> rec;
    std::vector<ctag_pose_cov_rec> cov;
    rig_records("calibrateHandEye", posesPerFrame, covPerFrame, nRigs, CTAG_HAND_EYE_MAX_ITEMS, nullptr, rec, cov);
    const size_t n_frames = posesPerFrame.size(), n = rec.size();
    if (links.size() != n_frames) throw std::string("calibrateHandEye, one link pose per frame\n");
    std::vector<ctag_link_pose> lk(n_frames);
    for (size_t f = 0; f < n_frames; f++)
        for (int k = 0; k < 3; k++) {
            lk[f].rvec[k] = links[f].rvec[k];
            lk[f].tvec[k] = links[f].tvec[k];
        }
    CountRigs set(nRigs);
    int st = set.status;
    std::vector<ctag_hand_eye_rec> out((size_t)nRigs);
    std::vector<ctag_hand_eye_frame_rec> fr(n);
    if (st == CTAG_OK) st = ctag_rig_hand_eye_fit(h_, set.rigs, rec.data(), cov.data(), (int)n_frames, lk.data(), opts, out.data(), fr.data());
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
    result.assign((size_t)nRigs, HandEyeInfo());
    for (int g = 0; g < nRigs; g++) {
        const ctag_hand_eye_rec& r = out[g];
        HandEyeInfo& hi = result[g];
        hi.rigID = r.rig;
        hi.status = r.status;
        hi.nUsed = r.n_used;
        hi.nDownweighted = r.n_downweighted;
        hi.rounds = r.rounds;
        hi.dof = r.dof;
        for (int k = 0; k < 3; k++) {
            hi.P.rvec[k] = r.P.rvec[k];
            hi.P.tvec[k] = r.P.tvec[k];
            hi.Q.rvec[k] = r.Q.rvec[k];
            hi.Q.tvec[k] = r.Q.tvec[k];
        }
        hi.cost0 = r.cost0;
        hi.cost = r.cost;
        hi.lambda = r.lambda;
        hi.sigma2Hat = r.sigma2_hat;
        hi.minPivot = r.min_pivot;
        for (int k = 0; k < 144; k++) hi.cov[k] = r.cov[k];
        hi.frames.assign(n_frames, HandEyeFrameInfo());
        for (size_t f = 0; f < n_frames; f++) {
            const ctag_hand_eye_frame_rec& q = fr[f * nRigs + g];
            HandEyeFrameInfo& fi = hi.frames[f];
            fi.status = q.status;
            fi.used = (q.flags & CTAG_HE_FLAG_USED) != 0;
            fi.downweighted = (q.flags & CTAG_HE_FLAG_DOWNWEIGHTED) != 0;
            for (int k = 0; k < 6; k++) fi.e[k] = q.e[k];
            fi.mahalanobis2 = q.mahalanobis2;
            fi.weight = q.weight;
        }
    }
}

static void pose_vectors(const PoseInfo& p, double* r, double* t) {
#ifdef CTAG_WITH_OPENCV
    const double *pr = p.rvec.ptr<double>(0), *pt = p.tvec.ptr<double>(0);
#else
    const double *pr = p.rvec, *pt = p.tvec;
#endif
    for (int i = 0; i < 3; i++) {
        r[i] = pr[i];
        t[i] = pt[i];
    }
}

// reference: CylinderTag::drawAxis, CylinderTag.cpp:211-246 (the overlay of include/ctag_pose.h: ctag_draw_axis)
void CylinderTag::drawAxis(const Mat& img, const std::vector<MarkerInfo>& markers, const std::vector<ModelInfo>& reconstruct_model,
                           const std::vector<PoseInfo>& pose, const CamInfo& camera, int axisLength, unsigned char* out, size_t out_step) {
    if (img.empty() || img.channels() != 1) throw std::string("drawAxis, the image must be 8-bit gray (cvtColor GRAY2RGB)\n");
    if (!out || out_step < (size_t)img.cols * 3) throw std::string("drawAxis, bad output buffer\n");
    if (markers.size() > (size_t)CTAG_MAX_MARKERS) throw std::string("drawAxis, more than 100 markers\n");
    ctag_frame_result res;
    if (flatten(markers, 0, res) != markers.size()) throw std::string("drawAxis, more than 100 features\n");
    // pose[i] with markers[i]: the reference's pairing by list position (poses past the end of the marker list draw nothing)
    std::vector<ctag_pose_rec> rec;
    for (size_t i = 0; i < pose.size() && i < markers.size(); i++) {
        ctag_pose_rec p;
        std::memset(&p, 0, sizeof(p));
        p.status = CTAG_POSE_OK;
        p.model_index = pose[i].markerID;
        p.frame = 0;
        p.marker = (int32_t)i;
        pose_vectors(pose[i], p.rvec, p.tvec);
        rec.push_back(p);
    }
    ctag_model* model = make_model(reconstruct_model, __FUNCTION__);
    const ctag_camera cam = make_camera(camera);
    const int st = ctag_draw_axis(h_, img.data, img.rows, img.cols, (ptrdiff_t)(size_t)img.step, &res, rec.data(), (int)rec.size(), model, &cam,
                                  axisLength, out, (ptrdiff_t)out_step);
    ctag_model_free(model);
    if (st != CTAG_OK) throw __FUNCTION__ + std::string(", ") + ctag_strerror(st) + "\n";
}

void CylinderTag::drawAxis(const Mat& img, std::vector<MarkerInfo> markers, std::vector<ModelInfo> reconstruct_model, std::vector<PoseInfo>& pose,
                           CamInfo camera, int axisLength) {
    AxisImage im;
    im.rows = img.rows;
    im.cols = img.cols;
    im.px.assign((size_t)img.rows * img.cols * 3, 0);
    drawAxis(img, markers, reconstruct_model, pose, camera, axisLength, im.px.data(), (size_t)img.cols * 3);
    axis_image_ = std::move(im);  // what the reference passes to imshow("Plot", imgMark)
}
