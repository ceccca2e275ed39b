// ctag_lm.h -- the decision that ends one Levenberg-Marquardt round of one group, stated once for the host loops of the four fits
// (ctag_fit_host.h, Lm::decide) and for the track smoother, which decides on the device (k_track.hip, k_track_decide).
#pragma once
#include "ctag_math.h"

namespace ctag {

struct LmState {
    double lambda, cost;  // the damping and the cost of the accepted state
    int active, rounds;
};

// One round is over.  A usable trial that lowers the cost is accepted: lambda / 3 (not below 1e-9), and the group stops when the
// drop is below rel_tol of the new cost.  Otherwise lambda x 4, and the group stops above lambda_max.  It stops after max_rounds
// rounds either way.  Returns whether the trial is accepted.
CTM_HD bool lm_decide(LmState& s, bool trial_usable, double cost_trial, double rel_tol, double lambda_max, int max_rounds) {
    s.rounds++;
    const bool accept = trial_usable && cost_trial < s.cost;
    if (accept) {
        const double drop = s.cost - cost_trial;
        s.cost = cost_trial;
        const double l3 = s.lambda / 3.0;
        s.lambda = l3 < 1e-9 ? 1e-9 : l3;
        if (drop < rel_tol * s.cost) s.active = 0;
    } else {
        s.lambda *= 4.0;
        if (s.lambda > lambda_max) s.active = 0;
    }
    if (s.rounds >= max_rounds) s.active = 0;
    return accept;
}

}  // namespace ctag
