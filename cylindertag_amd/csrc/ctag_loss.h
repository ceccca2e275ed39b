// ctag_loss.h -- Ceres 2.0's stock Huber and Cauchy losses on a squared norm s, stated once for the kernels that minimise under a
// loss: the robust refit (k_pose_robust.hip, s = a point's squared reprojection residual), the track smoother (k_track.hip, s = a
// frame's squared Mahalanobis norm) and the track filter (k_track_filter.hip, s = the innovation's).  Device only.
#pragma once
#include "../../include/ctag_pose.h"
#include "ctag_math.h"

namespace ctag {

// rule 5: rho(s) and rho'(s) for the loss's scale a (a2 = a * a, both positive)
__device__ __forceinline__ void robust_loss(int loss, double a, double a2, double s, double& rho, double& w) {
    if (loss == CTAG_LOSS_HUBER) {
        if (s <= a2) {
            rho = s;
            w = 1.0;
        } else {
            const double q = ctm::sqrt64(s);
            rho = 2.0 * a * q - a2;
            w = a / q;
        }
    } else {
        const double q = 1.0 + s / a2;
        rho = a2 * ctm::log64(q);
        w = 1.0 / q;
    }
}

}  // namespace ctag
