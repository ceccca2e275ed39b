// ctag_modelcheck.cpp -- the model calls of the C++ class (CylinderTag::saveModel, CylinderTag::reconstructModel), for
// tests/test_model_fit_cpp_gpu.py: the fixture model survives saveModel -> loadModel bit for bit, saveModel throws where it cannot
// write, and reconstructModel on the markers of one image seen three times returns a model list of the seed's shape whose unseen
// models are the seed's.
//   ctag_modelcheck <dictionary.marker> <image.bmp> <model.model> <cameraParams.yml> <dir for scratch files>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/CylinderTag.h"
#include "../csrc/ctag_io.h"

static bool same_bits(const std::vector<ModelInfo>& a, const std::vector<ModelInfo>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i].MarkerID != b[i].MarkerID || a[i].corners.size() != b[i].corners.size()) return false;
        if (std::memcmp(&a[i].base, &b[i].base, sizeof(a[i].base)) || std::memcmp(&a[i].axis, &b[i].axis, sizeof(a[i].axis))) return false;
        if (std::memcmp(a[i].corners.data(), b[i].corners.data(), sizeof(a[i].corners[0]) * a[i].corners.size())) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: ctag_modelcheck dictionary.marker image.bmp model.model cameraParams.yml scratch_dir\n");
        return 2;
    }
    try {
        CylinderTag t(argv[1]);
        std::vector<ModelInfo> fixture, back;
        t.loadModel(argv[3], fixture);
        const std::string dir = argv[5];
        t.saveModel(dir + "/copy.model", fixture);
        t.loadModel(dir + "/copy.model", back);
        std::printf("roundtrip %s models %zu\n", same_bits(fixture, back) ? "same" : "DIFFERENT", fixture.size());
        try {
            t.saveModel(dir + "/no/such/dir/x.model", fixture);
            std::printf("nothrow saveModel\n");
        } catch (const std::string& s) {
            std::printf("threw saveModel: %s", s.c_str());
        }
        CamInfo camera;
        t.loadCamera(argv[4], camera);
        const ctag_host::GrayImage g = ctag_host::read_bmp_gray(argv[2]);
        std::vector<MarkerInfo> markers;
        t.detect(ctag_host::Mat(g.rows, g.cols, g.px.data()), markers, 5, true, 5);
        std::vector<PoseInfo> pose;
        t.estimatePose(ctag_host::Mat(g.rows, g.cols, g.px.data()), markers, fixture, camera, pose);
        std::vector<bool> seen(fixture.size(), false);
        for (const PoseInfo& p : pose)
            if (p.markerID >= 0 && (size_t)p.markerID < seen.size()) seen[(size_t)p.markerID] = true;
        const std::vector<std::vector<MarkerInfo>> frames(3, markers);
        std::vector<ModelInfo> fitted;
        t.reconstructModel(frames, fixture, camera, fitted);
        std::printf("fitted models %zu\n", fitted.size());
        for (size_t i = 0; i < fitted.size() && i < fixture.size(); i++) {
            double worst = 0.0;
            bool finite = fitted[i].corners.size() == fixture[i].corners.size();
            for (size_t j = 0; finite && j < fitted[i].corners.size(); j++) {
                const double d[3] = {(double)fitted[i].corners[j].x - fixture[i].corners[j].x, (double)fitted[i].corners[j].y - fixture[i].corners[j].y,
                                     (double)fitted[i].corners[j].z - fixture[i].corners[j].z};
                for (double v : d) {
                    finite = finite && std::isfinite(v);
                    worst = std::fabs(v) > worst ? std::fabs(v) : worst;
                }
            }
            std::printf("model %zu id %d seen %d finite %d moved %.6g\n", i, fitted[i].MarkerID, (int)seen[i], (int)finite, worst);
        }
        std::vector<ModelInfo> again;
        t.saveModel(dir + "/fitted.model", fitted);
        t.loadModel(dir + "/fitted.model", again);
        std::printf("fitted roundtrip %s\n", same_bits(fitted, again) ? "same" : "DIFFERENT");
        try {
            t.reconstructModel({}, fixture, camera, fitted);
            std::printf("nothrow reconstructModel\n");
        } catch (const std::string& s) {
            std::printf("threw reconstructModel: %s", s.c_str());
        }
    } catch (const std::string& s) {
        std::printf("FAILED: %s", s.c_str());
        return 1;
    }
    return 0;
}
