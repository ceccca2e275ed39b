// ctag_tracknoisecheck.cpp -- the track noise fit through the C++ class (CylinderTag::calibrateTrackNoise, then startRigTracking with the
// fitted values), for tests/test_track_noise_cpp_gpu.py: the test writes the per-frame rig poses and covariances as the class returns
// them, the class fits the noise levels and then filters the same frames with the first result, and both come back as files of the C
// records, so that the test can hold them against the C calls byte for byte.
//   ctag_tracknoisecheck <dictionary.marker> <in.bin> <noise_opts.bin> <filter_opts.bin> <noise.bin> <track.bin>
// in.bin: as ctag_trackcheck's.  noise_opts.bin: one ctag_track_noise_opts.  filter_opts.bin: one ctag_track_filter_opts.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/CylinderTag.h"
#include "ctag_pose.h"

static ctag_track_rec as_record(const TrackInfo& t) {
    ctag_track_rec r = {};
    r.status = t.status;
    r.rig = t.rigID;
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

static ctag_track_noise_rec as_noise_record(const TrackNoiseInfo& n) {
    ctag_track_noise_rec r = {};
    r.status = n.status;
    r.rig = n.rigID;
    r.n_terms = n.nTerms;
    r.n_free = n.nFree;
    r.rounds = n.rounds;
    r.flags = n.flags;
    r.q_rot = n.qRot;
    r.q_trans = n.qTrans;
    r.cov_scale = n.covScale;
    for (int k = 0; k < 3; k++) r.log2_sigma[k] = n.log2Sigma[k];
    r.score = n.score;
    r.score_start = n.scoreStart;
    r.mean_m2 = n.meanM2;
    return r;
}

template <class T>
static bool write_records(const char* path, const std::vector<T>& out) {
    FILE* f = std::fopen(path, "wb");
    const bool ok = f && std::fwrite(out.data(), sizeof(T), out.size(), f) == out.size();
    if (f) std::fclose(f);
    return ok;
}

template <class T>
static bool read_one(const char* path, T& v) {
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(&v, sizeof(T), 1, f) == 1;
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: ctag_tracknoisecheck dictionary.marker in.bin noise_opts.bin filter_opts.bin noise.bin track.bin\n");
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
    ctag_track_noise_opts nopts;
    ctag_track_filter_opts fopts;
    if (!read_one(argv[3], nopts) || !read_one(argv[4], fopts)) return 2;
    try {
        CylinderTag tag{std::string(argv[1])};
        std::vector<TrackNoiseInfo> noise;
        tag.calibrateTrackNoise(poses, covs, n_rigs, noise, times, &nopts);
        std::vector<ctag_track_noise_rec> nrec;
        for (const TrackNoiseInfo& n : noise) nrec.push_back(as_noise_record(n));
        if (noise.empty() || !write_records(argv[5], nrec)) return 2;
        try {  // an option the fit refuses
            ctag_track_noise_opts bad = nopts;
            bad.rounds = 17;
            tag.calibrateTrackNoise(poses, covs, n_rigs, noise, times, &bad);
            std::printf("no throw\n");
        } catch (const std::string& e) {
            std::printf("threw %s", e.c_str());
        }
        tag.startRigTracking(n_rigs, noise[0], &fopts);
        std::vector<TrackInfo> track;
        std::vector<ctag_track_rec> out;
        for (int fr = 0; fr < n_frames; fr++) {
            if (times.empty()) tag.trackRigs(poses[fr], covs[fr], track);
            else tag.trackRigs(poses[fr], covs[fr], times[fr], track);
            if ((int)track.size() != n_rigs) return 3;
            for (int g = 0; g < n_rigs; g++) out.push_back(as_record(track[g]));
        }
        if (!write_records(argv[6], out)) return 2;
        std::printf("frames %d rigs %d searches %d\n", n_frames, n_rigs, (int)nrec.size());
        tag.stopRigTracking();
    } catch (const std::string& e) {
        std::fprintf(stderr, "%s", e.c_str());
        return 1;
    }
    return 0;
}
