// ctag_intrinsicscheck.cpp -- the intrinsics fit of the C++ class (CylinderTag::calibrateCamera), for tests/test_intr_fit_cpp_gpu.py:
// detection records written by the test (a file of ctag_frame_result) become the marker lists detect() would have returned, the class
// fits the camera and prints it with 9 significant digits and its sigmas with 17, so that the test can hold them against the C call
// float for float and double for double.
//   ctag_intrinsicscheck <dictionary.marker> <records.bin> <model.model> <seed.yml> <free mask> <tie focal> <rig of model 0> ...
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
    if (argc < 8) {
        std::fprintf(stderr, "usage: ctag_intrinsicscheck dictionary.marker records.bin model.model seed.yml free_mask tie_focal rig_of_model...\n");
        return 2;
    }
    try {
        CylinderTag t(argv[1]);
        std::vector<std::vector<MarkerInfo>> lists;
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) throw std::string("records file\n");
        ctag_frame_result r;
        while (std::fread(&r, sizeof(r), 1, f) == 1) lists.push_back(markers_of(r));
        std::fclose(f);
        std::vector<ModelInfo> model;
        t.loadModel(argv[3], model);
        CamInfo seed, camera;
        t.loadCamera(argv[4], seed);
        const unsigned mask = (unsigned)std::strtoul(argv[5], nullptr, 0);
        const bool tie = std::atoi(argv[6]) != 0;
        std::vector<int> rig;
        for (int i = 7; i < argc; i++) rig.push_back(std::atoi(argv[i]));
        std::vector<double> sigma;
        const bool ok = t.calibrateCamera(lists, model, rig, seed, camera, &sigma, mask, tie);
        std::printf("views %zu fitted %d\n", lists.size(), ok ? 1 : 0);
#ifdef CTAG_WITH_OPENCV
        cv::Mat Kf, Df;
        camera.Intrinsic.convertTo(Kf, CV_32F);
        camera.distCoeffs.convertTo(Df, CV_32F);
        const float* K = Kf.ptr<float>(0);
        const float* D = Df.ptr<float>(0);
        const size_t nd = Df.total();
#else
        const float* K = camera.Intrinsic;
        const float* D = camera.distCoeffs.data();
        const size_t nd = camera.distCoeffs.size();
#endif
        std::printf("K");
        for (int i = 0; i < 9; i++) std::printf(" %.9g", K[i]);
        std::printf("\ndist");
        for (size_t i = 0; i < nd; i++) std::printf(" %.9g", D[i]);
        std::printf("\nsigma");
        for (double s : sigma) std::printf(" %.17g", s);
        std::printf("\n");
        try {
            rig.pop_back();
            rig.push_back(0);
            rig.push_back(0);
            t.calibrateCamera(lists, model, rig, seed, camera);
            std::printf("nothrow calibrateCamera\n");
        } catch (const std::string& s) {
            std::printf("threw calibrateCamera: %s", s.c_str());
        }
    } catch (const std::string& s) {
        std::printf("FAILED: %s", s.c_str());
        return 1;
    }
    return 0;
}
