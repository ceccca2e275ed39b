// ctag_trackfiltercheck.cpp -- live track filtering through the C++ class (CylinderTag::startRigTracking / trackRigs / predictRigs), for
// tests/test_track_filter_cpp_gpu.py: the test writes the per-frame rig poses and covariances as the class returns them, the class
// filters them one frame a call and the records come back as files of ctag_track_rec, so that the test can hold them against the C
// calls byte for byte.
//   ctag_trackfiltercheck <dictionary.marker> <in.bin> <opts.bin> <out.bin> <predict time> <predict.bin>
// in.bin: as ctag_trackcheck's.  opts.bin: one ctag_track_filter_opts.  predict.bin: predictRigs(predict time) after the last frame.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/CylinderTag.h"
#include "ctag_pose.h"

static ctag_track_rec as_record(const TrackInfo& t, int frame) {
    ctag_track_rec r = {};
    r.status = t.status;
    r.rig = t.rigID;
    r.frame = frame;
    r.flags = (t.measured ? CTAG_TRACK_FLAG_MEASURED : 0u) | (t.downweighted ? CTAG_TRACK_FLAG_DOWNWEIGHTED : 0u) | (t.gated ? CTAG_TRACK_FLAG_GATED : 0u) |
              (t.started ? CTAG_TRACK_FLAG_STARTED : 0u);
    for (int k = 0; k < 3; k++) {
        r.rvec[k] = t.rvec[k];
        r.tvec[k] = t.tvec[k];
        r.w[k] = t.w[k];
        r.v[k] = t.v[k];
    }
    for (int k = 0; k < 36; k++) r.cov[k] = t.cov[k];
    for (int k = 0; k < 6; k++) r.vel_sigma[k] = t.velSigma[k];
    r.mahalanobis2 = t.mahalanobis2;
    r.weight = t.weight;
    return r;
}

static bool write_records(const char* path, const std::vector<ctag_track_rec>& out) {
    FILE* f = std::fopen(path, "wb");
    const bool ok = f && std::fwrite(out.data(), sizeof(ctag_track_rec), out.size(), f) == out.size();
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: ctag_trackfiltercheck dictionary.marker in.bin opts.bin out.bin predict_time predict.bin\n");
        return 2;
    }
    FILE* f = std::fopen(argv[2], "rb");
    int32_t hd[4];
    if (!f || std::fread(hd, sizeof(hd), 1, f) != 1) return 2;
    const int n_frames = hd[0], n_rigs = hd[1];
    std::vector<double> times(hd[2] ? n_frames : 0);
    if (hd[2] && std::fread(times.data(), sizeof(double), times.size(), f) != times.size()) return 2;
    std::vector<std::vector<RigPoseInfo>> poses(n_frames);
    std::vector<std::vector<PoseCovInfo>> covs(n_frames);
    for (int fr = 0; fr < n_frames; fr++)
        for (int g = 0; g < n_rigs; g++) {
            double v[44];
            if (std::fread(v, sizeof(v), 1, f) != 1) return 2;
            if (v[0] == 0.0) continue;  // the rig was erased from this frame's list
            RigPoseInfo p;
            p.rigID = g;
#ifdef CTAG_WITH_OPENCV
            p.rvec = (cv::Mat_<double>(3, 1) << v[2], v[3], v[4]);
            p.tvec = (cv::Mat_<double>(3, 1) << v[5], v[6], v[7]);
#else
            for (int k = 0; k < 3; k++) {
                p.rvec[k] = v[2 + k];
                p.tvec[k] = v[5 + k];
            }
#endif
            PoseCovInfo c;
            c.markerID = g;
            c.status = (int)v[1];
            for (int k = 0; k < 36; k++) c.cov[k] = v[8 + k];
            poses[fr].push_back(p);
            covs[fr].push_back(c);
        }
    std::fclose(f);
    ctag_track_filter_opts opts;
    f = std::fopen(argv[3], "rb");
    if (!f || std::fread(&opts, sizeof(opts), 1, f) != 1) return 2;
    std::fclose(f);
    try {
        CylinderTag tag{std::string(argv[1])};
        std::vector<TrackInfo> track;
        try {
            tag.trackRigs(poses[0], covs[0], track);
            std::printf("no throw\n");
        } catch (const std::string& e) {
            std::printf("threw %s", e.c_str());
        }
        tag.startRigTracking(n_rigs, &opts);
        std::vector<ctag_track_rec> out;
        for (int fr = 0; fr < n_frames; fr++) {
            if (times.empty()) tag.trackRigs(poses[fr], covs[fr], track);
            else tag.trackRigs(poses[fr], covs[fr], times[fr], track);
            if ((int)track.size() != n_rigs) return 3;
            for (int g = 0; g < n_rigs; g++) out.push_back(as_record(track[g], 0));
        }
        tag.predictRigs(std::strtod(argv[5], nullptr), track);
        std::vector<ctag_track_rec> pred;
        for (int g = 0; g < (int)track.size(); g++) pred.push_back(as_record(track[g], 0));
        if (!write_records(argv[4], out) || !write_records(argv[6], pred)) return 2;
        std::printf("frames %d rigs %d\n", n_frames, n_rigs);
        try {  // a time that does not exceed the last one
            tag.trackRigs(poses[0], covs[0], -1.0, track);
            std::printf("no throw\n");
        } catch (const std::string& e) {
            std::printf("threw %s", e.c_str());
        }
        tag.stopRigTracking();
    } catch (const std::string& e) {
        std::fprintf(stderr, "%s", e.c_str());
        return 1;
    }
    return 0;
}
