// ctag_handeyecheck.cpp -- hand-eye calibration through the C++ class (CylinderTag::calibrateHandEye), for tests/test_hand_eye_cpp_gpu.py:
// the test writes the per-frame rig poses and covariances as the class returns them and a link pose per frame, the class fits them and
// the records come back as two files of ctag_hand_eye_rec and ctag_hand_eye_frame_rec, so that the test can hold them against the C call
// byte for byte.
//   ctag_handeyecheck <dictionary.marker> <in.bin> <opts.bin> <out.bin> <frames.bin>
// in.bin: int32 n_frames, n_rigs, reserved[2]; n_frames x 6 doubles: the links' rvec, tvec; per (frame, rig) 44 doubles: present, cov
// status, rvec[3], tvec[3], cov[36].  opts.bin: one ctag_hand_eye_opts.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/CylinderTag.h"
#include "ctag_pose.h"

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: ctag_handeyecheck dictionary.marker in.bin opts.bin out.bin frames.bin\n");
        return 2;
    }
    FILE* f = std::fopen(argv[2], "rb");
    int32_t hd[4];
    if (!f || std::fread(hd, sizeof(hd), 1, f) != 1) return 2;
    const int n_frames = hd[0], n_rigs = hd[1];
    std::vector<LinkPose> links(n_frames);
    for (int fr = 0; fr < n_frames; fr++) {
        double v[6];
        if (std::fread(v, sizeof(v), 1, f) != 1) return 2;
        for (int k = 0; k < 3; k++) {
            links[fr].rvec[k] = v[k];
            links[fr].tvec[k] = v[3 + k];
        }
    }
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
    ctag_hand_eye_opts opts;
    f = std::fopen(argv[3], "rb");
    if (!f || std::fread(&opts, sizeof(opts), 1, f) != 1) return 2;
    std::fclose(f);
    try {
        CylinderTag tag{std::string(argv[1])};
        std::vector<HandEyeInfo> res;
        tag.calibrateHandEye(poses, covs, links, n_rigs, res, &opts);
        std::vector<ctag_hand_eye_rec> out((size_t)n_rigs);
        std::vector<ctag_hand_eye_frame_rec> frames((size_t)n_frames * n_rigs);
        for (int g = 0; g < n_rigs; g++) {
            const HandEyeInfo& h = res[g];
            ctag_hand_eye_rec r = {};
            r.status = h.status;
            r.rig = h.rigID;
            r.n_used = h.nUsed;
            r.n_downweighted = h.nDownweighted;
            r.rounds = h.rounds;
            r.dof = h.dof;
            for (int k = 0; k < 3; k++) {
                r.P.rvec[k] = h.P.rvec[k];
                r.P.tvec[k] = h.P.tvec[k];
                r.Q.rvec[k] = h.Q.rvec[k];
                r.Q.tvec[k] = h.Q.tvec[k];
            }
            r.cost0 = h.cost0;
            r.cost = h.cost;
            r.lambda = h.lambda;
            r.sigma2_hat = h.sigma2Hat;
            r.min_pivot = h.minPivot;
            for (int k = 0; k < 144; k++) r.cov[k] = h.cov[k];
            out[g] = r;
            for (int fr = 0; fr < n_frames; fr++) {
                const HandEyeFrameInfo& q = h.frames[fr];
                ctag_hand_eye_frame_rec fr_rec = {};
                fr_rec.status = q.status;
                fr_rec.rig = g;
                fr_rec.frame = fr;
                fr_rec.flags = (q.used ? CTAG_HE_FLAG_USED : 0u) | (q.downweighted ? CTAG_HE_FLAG_DOWNWEIGHTED : 0u);
                for (int k = 0; k < 6; k++) fr_rec.e[k] = q.e[k];
                fr_rec.mahalanobis2 = q.mahalanobis2;
                fr_rec.weight = q.weight;
                frames[(size_t)fr * n_rigs + g] = fr_rec;
            }
        }
        f = std::fopen(argv[4], "wb");
        if (!f || std::fwrite(out.data(), sizeof(ctag_hand_eye_rec), out.size(), f) != out.size()) return 2;
        std::fclose(f);
        f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(frames.data(), sizeof(ctag_hand_eye_frame_rec), frames.size(), f) != frames.size()) return 2;
        std::fclose(f);
        std::printf("frames %d rigs %d\n", n_frames, n_rigs);
        for (int bad = 0; bad < 3; bad++) {  // what the class refuses
            try {
                std::vector<HandEyeInfo> r2;
                if (bad == 0) tag.calibrateHandEye({}, {}, {}, n_rigs, r2);
                if (bad == 1) tag.calibrateHandEye(poses, covs, std::vector<LinkPose>(links.begin(), links.end() - 1), n_rigs, r2);
                if (bad == 2) {
                    ctag_hand_eye_opts o = opts;
                    o.mode = 2;
                    tag.calibrateHandEye(poses, covs, links, n_rigs, r2, &o);
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
