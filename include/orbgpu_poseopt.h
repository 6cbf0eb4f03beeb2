/*
 * orbgpu_poseopt.h -- C ABI of the motion-only pose optimisation
 * (Optimizer::PoseOptimization), batched: one frame pose per job, refined
 * against its MapPoint observations, with the inlier/outlier classification
 * that becomes Frame::mvbOutlier.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Optimizer::PoseOptimization              src/Optimizer.cpp:291-513
 *   OptimizationAlgorithmLevenberg::solve    Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
 *   BaseUnaryEdge::constructQuadraticForm    Thirdparty/g2o/g2o/core/base_unary_edge.hpp:43-72
 *   RobustKernelHuber                        Thirdparty/g2o/g2o/core/robust_kernel_impl.h:85, .cpp:64-91
 *   OptimizableGraph::Edge::robustInformation  Thirdparty/g2o/g2o/core/base_edge.h:96-102
 *   Edge(Stereo)SE3ProjectXYZOnlyPose        Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp} (.cpp:285-385)
 *   SE3Quat::exp, map, operator*             Thirdparty/g2o/g2o/types/se3quat.h:104-110, 217-257, 280-285
 * Callers: Tracking.cpp:1000 (TrackReferenceKeyFrame), :1167
 * (TrackWithMotionModel), :1225 (TrackLocalMap), :1852/:1869/:1884
 * (Relocalization).  Local and global bundle adjustment are not covered.
 *
 * What is restated: four rounds that each start from Tcw0 and run at most ten
 * Levenberg-Marquardt iterations of at most ten trials over the edges not
 * flagged by the round before (lambda0 = 1e-5 max|Hjj|, ni = 2, the 1/3..2/3
 * clamp, ORB-SLAM2's three-in-a-row stop rule); Huber kernels in rounds 0-2
 * (delta = (float)sqrt(5.991 | 7.815), dsqr in float) and none in round 3;
 * the stereo projection's invz, a double quotient rounded to float once
 * ((float)(1.0 / z), types_six_dof_expmap.cpp:320); the classification
 * (float)chi2 > (float)5.991 | 7.815 that reads an active edge's error from
 * the last trial (accepted or not) and a flagged edge's at the restored
 * estimate; one round only for fewer than 10 observations, none for fewer
 * than 3.  All arithmetic is double, as g2o's.
 *
 * Deviations (the comparison with a g2o build is unpinned: g2o needs Eigen,
 * DESIGN.md):
 *   - the dense 6x6 solve is a Cholesky factorisation without pivoting, not
 *     Eigen::LDLT; a pivot that is not positive is the failed solve;
 *   - after a failed solve the reference applies the stale previous x before
 *     it pops the estimate; here a failed solve is a rejected zero step;
 *   - pow(theta, 3) of SE3Quat::exp is theta*theta*theta; the quaternion
 *     algebra is Eigen 3's as recalled.
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error().
 */
#ifndef ORBGPU_POSEOPT_H
#define ORBGPU_POSEOPT_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame.  An observation is one keypoint with a non-null MapPoint; the
 * caller gathers them (as PnPsolver's constructor gathers its
 * correspondences).  Observations [offset, offset + n) of the batch arrays:
 *   Xw          float[3]: pMP->GetWorldPos()
 *   obs         float[3]: mvKeysUn[i].pt.x, .pt.y, mvuRight[i]; uRight < 0
 *               makes the monocular edge (2 residuals), otherwise the stereo
 *               edge (3 residuals)
 *   inv_sigma2  float: mvInvLevelSigma2[mvKeysUn[i].octave]
 * Ranges of different jobs must not overlap. */
typedef struct orbgpu_poseopt_job {
    int n, offset;
    float Tcw0[12];       /* pFrame->mTcw, row-major 3x4 [R|t]                      */
    float fx, fy, cx, cy, bf;
    int pad;
} orbgpu_poseopt_job;

typedef struct orbgpu_poseopt_result {
    int n_good;           /* the reference's return value: nInitialCorrespondences - nBad */
    int rounds;           /* outer rounds run: 0 (n < 3), 1 (n < 10), else 4        */
    int lm_iterations[4]; /* diagnostics: LM iterations (solve() calls) and rejected */
    int lm_rejected[4];   /* trials per round; they depend on rounding noise at convergence */
    float Tcw[16];        /* row-major 4x4; Tcw0 made homogeneous when n < 3        */
} orbgpu_poseopt_result;

/* Batched, HBM-resident (jobs included), asynchronous on `stream`; one
 * workgroup per job, the whole optimisation inside one launch.
 * d_outlier[offset + i] is mvbOutlier of that observation after the call
 * (0 / 1; all 0 when n < 3); bytes outside every job's range are not written.
 * A job's result and flags do not depend on the batch it runs in or on its
 * position, and repeat bit for bit from call to call.
 * ORBGPU_ERR_ARG, checked before the device is: batch < 0, total_obs < 0, a
 * NULL d_jobs / d_results with batch > 0, a NULL observation array or
 * d_outlier with batch > 0 and total_obs > 0.  The jobs live on the device, so
 * their ranges cannot be checked here: a job with n < 0, offset < 0 or
 * offset + n > total_obs reads and writes no observation and gets
 * n_good = rounds = -1, while the call still returns ORBGPU_OK. */
int orbgpu_pose_optimization_batch_device(int batch, const orbgpu_poseopt_job* d_jobs, int total_obs,
                                          const float* d_Xw, const float* d_obs, const float* d_inv_sigma2,
                                          orbgpu_poseopt_result* d_results, uint8_t* d_outlier, void* stream);
/* Host-pointer form (uploads, runs, downloads, synchronises).  The argument
 * checks above, and per job n < 0, offset < 0 or offset + n > total_obs, are
 * ORBGPU_ERR_ARG before the device is looked at.  batch == 0 succeeds without
 * a device; so does total_obs == 0, where every job has n == 0 and its result
 * (n_good = rounds = 0, Tcw0 made homogeneous) is written by the host. */
int orbgpu_pose_optimization_batch(int batch, const orbgpu_poseopt_job* jobs, int total_obs, const float* Xw,
                                   const float* obs, const float* inv_sigma2, orbgpu_poseopt_result* results,
                                   uint8_t* outlier);

#ifdef __cplusplus
}
#endif
#endif
