/*
 * orbgpu_sim3opt.h -- C ABI of the Sim3 refinement of a loop candidate
 * (Optimizer::OptimizeSim3), batched: one relative Sim3 S12 per job, refined
 * against its MapPoint correspondences by reprojection in both keyframes, with
 * the flags that become vpMatches1[idx] = NULL and the inlier count that
 * LoopClosing::ComputeSim3 compares with 20.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Optimizer::OptimizeSim3                  src/Optimizer.cpp:1229-1433 (caller: src/LoopClosing.cpp:393)
 *   EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ, VertexSim3Expmap::oplusImpl, cam_map1/2
 *                                            Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:61-90, 131-172
 *   Sim3(Vector7d), map, inverse, operator*  Thirdparty/g2o/g2o/types/sim3.h:70-146, 233-236, 266-272
 *   BaseBinaryEdge::linearizeOplus (numeric), constructQuadraticForm
 *                                            Thirdparty/g2o/g2o/core/base_binary_edge.hpp:131-204, 91-113
 *   RobustKernelHuber, robustInformation     Thirdparty/g2o/g2o/core/robust_kernel_impl.{h,cpp}, base_edge.h:96-102
 *   OptimizationAlgorithmLevenberg::solve    Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
 *   Converter::toCvMat(g2o::Sim3)            src/Converter.cpp:55-61
 *
 * What is restated.  Both MapPoint vertices of a correspondence are fixed, so
 * the only unknown is the 7-vector update of S12 = (q, t, s).  Per
 * correspondence two edges: e12 = obs1 - cam_map1(project(S.map(P2c))) and
 * e21 = obs2 - cam_map2(project(S.inverse().map(P1c))), chi2 = e . (w e).
 * Neither edge has an analytic Jacobian: column d is
 * (e(oplus(+1e-9 e_d)) - e(oplus(-1e-9 e_d))) * (1 / 2e-9), oplus(u) =
 * Sim3(u) * S with u[6] = 0 under fix_scale and the four branches of
 * Sim3(Vector7d) on |sigma| < 1e-5 and theta < 1e-5; quaternion products are
 * not normalised.  Huber on both edges in both optimisations, delta =
 * (float)sqrt(th2), dsqr in float; rho[1] w as the information, b += J^T
 * (rho[1] (-(w e))).  optimize(5) over all correspondences; a pair with
 * e12.chi2 > th2 || e21.chi2 > th2 (as written: a NaN is not flagged) is
 * removed; fewer than 10 left: return 0, S12 untouched; otherwise
 * optimize(nBad > 0 ? 10 : 5) over the survivors from the estimate the first
 * left (lambda, ni and the stop counter start afresh), the same check again,
 * nIn the survivors that pass.  Both checks read each edge's error from the
 * last trial evaluated, accepted or not.  Under fix_scale the seventh column
 * is exactly zero and s12 keeps its bits: a consequence of the arithmetic
 * (Sim3(0) is the exact identity), not a special case.  All arithmetic is
 * double, as g2o's.
 *
 * Deviations (the comparison with a g2o build is unpinned: g2o needs Eigen,
 * DESIGN.md §5g):
 *   - the dense 7x7 solve is a Cholesky factorisation without pivoting, not
 *     Eigen::LDLT; a pivot that is not positive is the failed solve;
 *   - after a failed solve the reference applies the stale previous x before
 *     it pops the estimate; here a failed solve is a rejected zero step;
 *   - the quaternion algebra (Quaterniond(Matrix3d), the product,
 *     _transformVector, conjugate, toRotationMatrix) is Eigen 3's as recalled;
 *   - Sim3::log is not needed and not restated.
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error().
 */
#ifndef ORBGPU_SIM3OPT_H
#define ORBGPU_SIM3OPT_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One OptimizeSim3 call.  A correspondence is one index i that passed the
 * gathers of Optimizer.cpp:1284-1366, in ascending i.  Correspondences
 * [offset, offset + n) of the batch arrays:
 *   P1c, P2c      float[3] each: R1w*P3D1w + t1w and R2w*P3D2w + t2w as the
 *                 caller's float cv::Mat product gave them (widened to double here)
 *   obs1, obs2    float[2] each: pKF1->mvKeysUn[i].pt, pKF2->mvKeysUn[i2].pt
 *   inv_sigma2_1, inv_sigma2_2   float each: mvInvLevelSigma2[octave]
 * Ranges of different jobs must not overlap. */
typedef struct orbgpu_sim3opt_job {
    int n, offset;
    double q12[4];        /* g2oS12.rotation(): x, y, z, w                           */
    double t12[3];        /* g2oS12.translation()                                    */
    double s12;           /* g2oS12.scale()                                          */
    float K1[4], K2[4];   /* fx, fy, cx, cy of pKF1->mK, pKF2->mK                    */
    float th2;
    int fix_scale;        /* bFixScale                                               */
} orbgpu_sim3opt_job;

typedef struct orbgpu_sim3opt_result {
    int n_in;             /* the reference's return value                            */
    int rounds;           /* optimisations run: 0 (n == 0), 1 (fewer than 10 survivors), 2 */
    int n_bad_first;      /* nBad of the first check                                 */
    int lm_iterations[2]; /* diagnostics: LM iterations (solve() calls) and rejected */
    int lm_rejected[2];   /* trials; they depend on rounding noise at convergence    */
    int pad;
    double q12[4], t12[3], s12; /* the estimate; the input's bits when rounds < 2   */
    float T12[16];        /* Converter::toCvMat(g2o::Sim3) of it: row-major [sR t; 0 1] */
} orbgpu_sim3opt_result;

/* Batched, HBM-resident (jobs included), asynchronous on `stream`; one
 * workgroup per job, both optimisations and both checks inside one launch.
 * d_removed[offset + k] is 1 where the reference sets vpMatches1[idx] = NULL
 * for correspondence k and 0 elsewhere in the job's range; bytes outside every
 * job's range are not written.  A job's result and flags do not depend on the
 * batch it runs in or on its position, and repeat bit for bit from call to call.
 * ORBGPU_ERR_ARG, checked before the device is: batch < 0, total_corr < 0, a
 * NULL d_jobs / d_results with batch > 0, a NULL correspondence array or
 * d_removed with batch > 0 and total_corr > 0.  The jobs live on the device,
 * so their ranges cannot be checked here: a job with n < 0, offset < 0 or
 * offset + n > total_corr reads and writes no correspondence and gets
 * n_in = rounds = -1, while the call still returns ORBGPU_OK. */
int orbgpu_optimize_sim3_batch_device(int batch, const orbgpu_sim3opt_job* d_jobs, int total_corr,
                                      const float* d_P1c, const float* d_P2c, const float* d_obs1,
                                      const float* d_obs2, const float* d_inv_sigma2_1,
                                      const float* d_inv_sigma2_2, orbgpu_sim3opt_result* d_results,
                                      uint8_t* d_removed, void* stream);
/* Host-pointer form (uploads, runs, downloads, synchronises).  The argument
 * checks above, and per job n < 0, offset < 0 or offset + n > total_corr, are
 * ORBGPU_ERR_ARG before the device is looked at.  batch == 0 succeeds without
 * a device; so does total_corr == 0, where every job has n == 0 and its result
 * (n_in = rounds = 0, the input estimate and its T12) is written by the host. */
int orbgpu_optimize_sim3_batch(int batch, const orbgpu_sim3opt_job* jobs, int total_corr, const float* P1c,
                               const float* P2c, const float* obs1, const float* obs2,
                               const float* inv_sigma2_1, const float* inv_sigma2_2,
                               orbgpu_sim3opt_result* results, uint8_t* removed);

#ifdef __cplusplus
}
#endif
#endif
