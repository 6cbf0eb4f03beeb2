// wholechip_lm.h -- what globalba.hip and essential.hip share for driving
// g2o's Levenberg-Marquardt (lm_runtime.h) from the host over one problem
// spread over the whole chip: the control block at the head of the workspace,
// the coherent pinned record the host reads once per trial, the fixed-order
// sums of per-lane and per-workgroup values, the launch with its check, and
// the bodies of the one-lane kernels that begin an iteration and judge a
// trial.  The host loops stay with each file: they launch different kernels.
// block_total is localba.hip's too.
#pragma once

#include <hip/hip_runtime.h>

#include "host_common.h"
#include "lm_runtime.h"

namespace orbgpu {
namespace wholechip {

// the optimisation's state on the device; zeroed by the call, then written by one lane of one kernel
// at a time.  A file may keep a control block of its own with these members among its own (globalba.hip
// has max_bits between run and first_chi); it fits kCtlBytes.
struct CtlBase {
    lm::Run run;
    double first_chi;
    int bad, fail, nf, n_active;
};
constexpr size_t kCtlBytes = 256;
static_assert(sizeof(CtlBase) <= kCtlBytes, "CtlBase outgrew its slot");

// what the host reads after a synchronisation (coherent pinned memory)
struct HostRec {
    double chi, first_chi, lambda;
    int bad, nf, n_active, solved, accepted, more, done, iter, rejected, pad;
};

// the calling thread's record, allocated at its first call and kept.  Every optimiser that includes this
// header uses the same one: their calls are synchronous and clear it on entry.
struct PinnedRec {
    HostRec* p = nullptr;
    ~PinnedRec() {
        if (p) (void)hipHostFree(p);
    }
};
inline int host_rec(HostRec** out) {
    thread_local PinnedRec r;
    if (!r.p) ORB_HIP(hipHostMalloc((void**)&r.p, sizeof(HostRec), hipHostMallocCoherent));
    *out = r.p;
    return ORBGPU_OK;
}

inline unsigned blocks_for(size_t lanes, int threads = 256) { return (unsigned)((lanes + threads - 1) / threads); }

// enqueue a kernel on `stream`; a launch error returns from the calling function
#define ORB_LAUNCH(stream, kernel, grid, block, ...)                      \
    do {                                                                  \
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);  \
        ORB_HIP(hipGetLastError());                                       \
    } while (0)

__device__ inline size_t global_tid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

// the workgroup's sum of one value per lane in lane order, in lane 0: 16 lanes add 16 values each,
// lane 0 adds the 16 sums
__device__ inline double block_total(double v, double (&s_val)[256], double (&s_row)[16]) {
    const int tid = threadIdx.x;
    s_val[tid] = v;
    __syncthreads();
    if (tid < 16) {
        double s = s_val[16 * tid];
        for (int k = 1; k < 16; ++k) s += s_val[16 * tid + k];
        s_row[tid] = s;
    }
    __syncthreads();
    double s = 0.0;
    if (tid == 0) {
        s = s_row[0];
        for (int k = 1; k < 16; ++k) s += s_row[k];
    }
    return s;
}

// the sum of n per-workgroup partial sums in workgroup order
__device__ inline double ordered_sum(const double* part, int n) {
    double s = 0.0;
    if (n > 0) {
        s = part[0];
        for (int k = 1; k < n; ++k) s += part[k];
    }
    return s;
}

// the iteration begins: the robust chi2 at the kept estimates; in the first, init_lambda(c.run) is
// the file's computeLambdaInit.  One lane.  The sum comes before every store, so that its loads
// stay scalar loads.
template <class Ctl, class InitLambda>
__device__ inline void begin_iteration(Ctl& c, const double* chi_part, int n_chi, int first,
                                       InitLambda&& init_lambda) {
    const double chi = ordered_sum(chi_part, n_chi);
    if (first) {
        init_lambda(c.run);
        c.first_chi = chi;
    }
    lm::run_begin_iteration(c.run, chi);
    c.fail = 0;
}

// OptimizationAlgorithmLevenberg::solve's decisions after a trial, by one lane; the host reads rec.
// After a failed solve the trial moved nothing: computeScale's sum is +0.0 and run_judge's rho comes
// from it, so the partial sums are not read.
template <class Ctl>
__device__ inline void judge(Ctl& c, HostRec* rec, const double* chi_part, int n_chi, const double* scale_part,
                             int n_scale, int max_iter) {
    const bool solved = !c.fail;
    const double tmp_chi = solved ? ordered_sum(chi_part, n_chi) : 0.0;
    const double ssum = solved ? ordered_sum(scale_part, n_scale) : 0.0;
    const bool accepted = lm::run_judge(c.run, solved, tmp_chi, ssum);
    const bool more = lm::run_more_trials(c.run);
    const bool done = more ? false : lm::run_end_iteration(c.run, max_iter);
    c.fail = 0;
    rec->chi = c.run.chi, rec->first_chi = c.first_chi, rec->lambda = c.run.lambda;
    rec->solved = solved, rec->accepted = accepted, rec->more = more, rec->done = done;
    rec->iter = c.run.iter, rec->rejected = c.run.rejected;
    __threadfence_system();
}

}  // namespace wholechip
}  // namespace orbgpu
