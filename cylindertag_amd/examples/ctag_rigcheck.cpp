// ctag_rigcheck.cpp -- the rig assembly of the C++ class (CylinderTag::assembleRigModel), for tests/test_rig_fit_cpp_gpu.py: detection
// records written by the test (a file of ctag_frame_result) become the marker lists detect() would have returned, the class assembles
// the model and saveModel writes it, so that the test can hold it against the C call float for float.
//   ctag_rigcheck <dictionary.marker> <records.bin> <model.model> <cameraParams.yml> <out.model> <rig of model 0> <rig of model 1> ...
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
    if (argc < 7) {
        std::fprintf(stderr, "usage: ctag_rigcheck dictionary.marker records.bin model.model cameraParams.yml out.model rig_of_model...\n");
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
        std::vector<std::vector<MarkerInfo>> frames;
        for (const ctag_frame_result& rec : recs) frames.push_back(markers_of(rec));
        std::vector<ModelInfo> model, out;
        t.loadModel(argv[3], model);
        CamInfo camera;
        t.loadCamera(argv[4], camera);
        std::vector<int> rig, placed;
        for (int i = 6; i < argc; i++) rig.push_back(std::atoi(argv[i]));
        t.assembleRigModel(frames, model, rig, camera, out, placed);
        t.saveModel(argv[5], out);
        std::printf("frames %zu models %zu placed", frames.size(), out.size());
        for (int g : placed) std::printf(" %d", g);
        std::printf("\n");
        try {
            t.assembleRigModel({}, model, rig, camera, out, placed);
            std::printf("nothrow assembleRigModel\n");
        } catch (const std::string& s) {
            std::printf("threw assembleRigModel: %s", s.c_str());
        }
        try {
            rig.pop_back();
            t.assembleRigModel(frames, model, rig, camera, out, placed);
            std::printf("nothrow assembleRigModel\n");
        } catch (const std::string& s) {
            std::printf("threw assembleRigModel: %s", s.c_str());
        }
    } catch (const std::string& s) {
        std::printf("FAILED: %s", s.c_str());
        return 1;
    }
    return 0;
}
