// lm_runtime.h -- the scalar decisions of g2o's Levenberg-Marquardt
// (core/optimization_algorithm_levenberg.cpp:61-189) for an optimiser whose
// number of unknowns is known at run time only (localba.hip).  lm_device.h's
// lm::step<N> makes the same decisions, but interleaved with its compile-time
// N x N solve and its register-resident system; they are restated here, with
// lm_device.h's constants, so that poseopt.hip and sim3opt.hip compile to the
// instructions they had.  tests/localba_ref.py's levenberg()
// is the same logic.  One lane advances a Run between barriers.
#pragma once

#include "lm_device.h"

namespace orbgpu {
namespace lm {

struct Run {
    double lambda, ni, chi, ini_chi, rho;
    int iter, qmax, stop_bad, rejected;
};

// optimize() from the current estimates: lambda, ni and the stop counter are set by the first build
__device__ inline void run_start(Run& r) {
    r.lambda = 0.0, r.ni = 0.0, r.chi = 0.0, r.ini_chi = 0.0, r.rho = 0.0;
    r.iter = 0, r.qmax = 0, r.stop_bad = 0, r.rejected = 0;
}

// computeLambdaInit after the first build; max_diag is the maximum of |H_jj| over the active vertices
__device__ inline void run_init_lambda(Run& r, double max_diag) {
    r.lambda = kTau * max_diag;
    r.ni = 2.0;
    r.stop_bad = 0;
}

// computeLambdaInit under setUserLambdaInit(user_lambda > 0) (:166-169): no diagonal maximum is taken
__device__ inline void run_init_lambda_user(Run& r, double user_lambda) {
    r.lambda = user_lambda;
    r.ni = 2.0;
    r.stop_bad = 0;
}

// a build pass gave the robust chi2 at the kept estimate: the iteration begins
__device__ inline void run_begin_iteration(Run& r, double chi) {
    r.chi = chi;
    r.iter += 1;
    r.ini_chi = chi;
    r.qmax = 0;
    r.rho = 0.0;
}

// one trial: tmp_chi is its robust chi2 (ignored after a failed solve), scale_sum is computeScale's
// sum without its guard.  True when the trial is accepted.
__device__ inline bool run_judge(Run& r, bool solved, double tmp_chi, double scale_sum) {
    if (!solved) tmp_chi = DBL_MAX;
    const double scale = scale_sum + kScaleGuard;
    const double rho = (r.chi - tmp_chi) / scale;
    r.rho = rho;
    bool accepted = false;
    if (rho > 0 && isfinite(tmp_chi)) {
        const double t3 = 2.0 * rho - 1.0;
        double alpha = 1.0 - (t3 * t3) * t3;
        alpha = alpha < kAlphaMax ? alpha : kAlphaMax;
        r.lambda *= (kAlphaMin < alpha ? alpha : kAlphaMin);
        r.ni = 2.0;
        r.chi = tmp_chi;
        accepted = true;
    } else {
        r.lambda *= r.ni;
        r.ni *= 2.0;
        r.rejected += 1;
    }
    r.qmax += 1;
    return accepted;
}

__device__ inline bool run_more_trials(const Run& r) { return r.rho < 0 && r.qmax < kMaxTrials; }

// after the iteration's last trial: true when the optimisation ends
__device__ inline bool run_end_iteration(Run& r, int max_iter) {
    if (r.qmax == kMaxTrials || r.rho == 0) return true;
    if ((r.ini_chi - r.chi) * kStopGain < r.ini_chi)
        r.stop_bad += 1;
    else
        r.stop_bad = 0;
    return r.stop_bad >= kMaxBadIterations || r.iter >= max_iter;
}

}  // namespace lm
}  // namespace orbgpu
