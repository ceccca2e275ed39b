// ctag_camsetcheck.cpp -- the camera set fit of the C++ class (CylinderTag::calibrateCameraSet), for tests/test_cam_fit_cpp_gpu.py:
// detection records written by the test (a file of ctag_frame_result, camera-major) become the marker lists detect() would have
// returned, the class fits the camera poses and prints them with 17 significant digits, so that the test can hold them against the C
// call double for double.
//   ctag_camsetcheck <dictionary.marker> <records.bin> <model.model> <n_cameras> <camera 0.yml> ... <rig of model 0> <rig of model 1> ...
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/CylinderTag.h"
#include "ctag_types.h"

// one detection record -> the list detect() returns for it (empty for a frame that is not CTAG_OK)
static std::vector<MarkerInfo> markers_of(const ctag_frame_result& r) {
    std::vector<MarkerInfo> out;
    if (r.status != CTAG_OK) return out;
    for (int m = 0; m < r.n_markers && m < CTAG_MAX_MARKERS; m++) {
        const ctag_marker_rec& M = r.markers[m];
        MarkerInfo mi;
        mi.markerID = M.marker_id;
        for (int j = 0; j < M.n_features && M.first_feature + j < CTAG_MAX_FEATURES; j++) {
            const ctag_feature_rec& F = r.features[M.first_feature + j];
            if (j < M.n_pos) mi.featurePos.push_back(F.pos);
            mi.feature_ID.push_back(F.id);
            mi.feature_ID_left.push_back(F.id_left);
            mi.feature_ID_right.push_back(F.id_right);
            std::vector<ctag_host::Point2f> c(8);
            for (int k = 0; k < 8; k++) c[k] = ctag_host::Point2f(F.corners[2 * k], F.corners[2 * k + 1]);
            mi.cornerLists.push_back(c);
        }
        out.push_back(mi);
    }
    return out;
}

int main(int argc, char** argv) {
    const int nc = argc > 4 ? std::atoi(argv[4]) : 0;
    if (nc < 1 || argc < 5 + nc + 1) {
        std::fprintf(stderr, "usage: ctag_camsetcheck dictionary.marker records.bin model.model n_cameras camera.yml... rig_of_model...\n");
        return 2;
    }
    try {
        CylinderTag t(argv[1]);
        std::vector<ctag_frame_result> recs;
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) throw std::string("records file\n");
        ctag_frame_result r;
        while (std::fread(&r, sizeof(r), 1, f) == 1) recs.push_back(r);
        std::fclose(f);
        const size_t nf = recs.size() / (size_t)nc;
        std::vector<std::vector<std::vector<MarkerInfo>>> lists((size_t)nc);
        for (int c = 0; c < nc; c++)
            for (size_t i = 0; i < nf; i++) lists[c].push_back(markers_of(recs[(size_t)c * nf + i]));
        std::vector<ModelInfo> model;
        t.loadModel(argv[3], model);
        std::vector<CamInfo> cameras((size_t)nc);
        for (int c = 0; c < nc; c++) t.loadCamera(argv[5 + c], cameras[c]);
        std::vector<int> rig, placed;
        for (int i = 5 + nc; i < argc; i++) rig.push_back(std::atoi(argv[i]));
        std::vector<ViewPose> poses;
        const bool all = t.calibrateCameraSet(lists, model, rig, cameras, poses, placed);
        std::printf("cameras %d instants %zu all %d\n", nc, nf, all ? 1 : 0);
        for (int c = 0; c < nc; c++) {
#ifdef CTAG_WITH_OPENCV
            const double *pr = poses[c].rvec.ptr<double>(0), *pt = poses[c].tvec.ptr<double>(0);
#else
            const double *pr = poses[c].rvec, *pt = poses[c].tvec;
#endif
            std::printf("camera %d placed %d pose %.17g %.17g %.17g %.17g %.17g %.17g\n", c, placed[c], pr[0], pr[1], pr[2], pt[0], pt[1], pt[2]);
        }
        try {
            std::vector<CamInfo> one(1);
            t.calibrateCameraSet(lists, model, rig, one, poses, placed);
            std::printf("nothrow calibrateCameraSet\n");
        } catch (const std::string& s) {
            std::printf("threw calibrateCameraSet: %s", s.c_str());
        }
        try {
            rig.pop_back();
            t.calibrateCameraSet(lists, model, rig, cameras, poses, placed);
            std::printf("nothrow calibrateCameraSet\n");
        } catch (const std::string& s) {
            std::printf("threw calibrateCameraSet: %s", s.c_str());
        }
    } catch (const std::string& s) {
        std::printf("FAILED: %s", s.c_str());
        return 1;
    }
    return 0;
}
