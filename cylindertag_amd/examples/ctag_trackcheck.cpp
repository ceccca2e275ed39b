// ctag_trackcheck.cpp -- track smoothing through the C++ class (CylinderTag::smoothRigTrack), for tests/test_track_cpp_gpu.py: the test
// writes the per-frame rig poses and covariances as the class returns them, the class smooths them and the records come back as a file
// of ctag_track_rec, so that the test can hold them against the C call byte for byte.
//   ctag_trackcheck <dictionary.marker> <in.bin> <opts.bin> <out.bin>
// in.bin: int32 n_frames, n_rigs, has_times, reserved; [n_frames doubles if has_times]; per (frame, rig) 44 doubles: present, cov status,
// rvec[3], tvec[3], cov[36].  opts.bin: one ctag_track_opts.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/CylinderTag.h"
#include "ctag_pose.h"

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: ctag_trackcheck dictionary.marker in.bin opts.bin out.bin\n");
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
    ctag_track_opts opts;
    f = std::fopen(argv[3], "rb");
    if (!f || std::fread(&opts, sizeof(opts), 1, f) != 1) return 2;
    std::fclose(f);
    try {
        CylinderTag tag{std::string(argv[1])};
        std::vector<std::vector<TrackInfo>> track;
        tag.smoothRigTrack(poses, covs, n_rigs, track, times, &opts);
        std::vector<ctag_track_rec> out((size_t)n_frames * n_rigs);
        for (int fr = 0; fr < n_frames; fr++)
            for (int g = 0; g < n_rigs; g++) {
                const TrackInfo& t = track[fr][g];
                ctag_track_rec r = {};
                r.status = t.status;
                r.rig = t.rigID;
                r.frame = fr;
                r.flags = (t.measured ? CTAG_TRACK_FLAG_MEASURED : 0u) | (t.downweighted ? CTAG_TRACK_FLAG_DOWNWEIGHTED : 0u);
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
                out[(size_t)fr * n_rigs + g] = r;
            }
        f = std::fopen(argv[4], "wb");
        if (!f || std::fwrite(out.data(), sizeof(ctag_track_rec), out.size(), f) != out.size()) return 2;
        std::fclose(f);
        std::printf("frames %d rigs %d\n", n_frames, n_rigs);
        for (int bad = 0; bad < 3; bad++) {  // what the class refuses
            try {
                std::vector<std::vector<TrackInfo>> t2;
                if (bad == 0) tag.smoothRigTrack({}, {}, n_rigs, t2);
                if (bad == 1) tag.smoothRigTrack(poses, std::vector<std::vector<PoseCovInfo>>(covs.begin(), covs.end() - 1), n_rigs, t2);
                if (bad == 2) {
                    ctag_track_opts o = opts;
                    o.max_gap = 0;
                    tag.smoothRigTrack(poses, covs, n_rigs, t2, times, &o);
                }
                std::printf("no throw %d\n", bad);
            } catch (const std::string& e) {
                std::printf("threw %s", e.c_str());
            }
        }
    } catch (const std::string& e) {
        std::fprintf(stderr, "%s", e.c_str());
        return 1;
    }
    return 0;
}
