/*
 * orbgpu_localba.h -- C ABI of the local bundle adjustment
 * (Optimizer::LocalBundleAdjustment), batched: one job is the optimisation of
 * one keyframe neighbourhood -- the local keyframe poses and the MapPoints
 * they see, against the observations of those points in the local and in the
 * fixed keyframes -- with the two rounds and the edge classification that
 * becomes the erased observations.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Optimizer::LocalBundleAdjustment         src/Optimizer.cpp:536-885 (the optimisation: :759-847)
 *   Edge(Stereo)SE3ProjectXYZ                Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:112-168, 199-245
 *   BaseBinaryEdge::constructQuadraticForm   Thirdparty/g2o/g2o/core/base_binary_edge.hpp:43-120
 *   BlockSolver::solve, setLambda            Thirdparty/g2o/g2o/core/block_solver.hpp:355-487, 565-610
 *   OptimizationAlgorithmLevenberg::solve    Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
 *   SparseOptimizer::initializeOptimization  Thirdparty/g2o/g2o/core/sparse_optimizer.cpp
 * Caller: LocalMapping::Run after every inserted keyframe.  The gather and the
 * write-back are include/orbslam2_amd/LocalBundleAdjuster.h's.
 *
 * What is restated: optimize(5) with Huber on every edge (delta =
 * (float)sqrt(5.991 | 7.815)); the test chi2 > 5.991 | 7.815 ||
 * !isDepthPositive() in double, which sends an edge to level 1; optimize(10)
 * without kernels from the current estimates with lambda, ni and the stop
 * counter afresh; the same test over all edges for the erase flags.  The active
 * set is initializeOptimization(0)'s: a point or a local pose that no level-0
 * edge touches is not optimised, not damped and not in the lambda maximum; an
 * edge to a fixed pose contributes to its point only.  An active edge's chi2 is
 * the error of the last trial evaluated, accepted or not; a level-1 edge's is
 * its stale first-round value while its depth test reads the final estimates.
 * Every local pose goes through Converter::toSE3Quat on the way in and
 * Converter::toCvMat(SE3Quat) on the way out, so a fixed local pose does not
 * in general keep its input bits.  All arithmetic is double, as g2o's.
 *
 * Deviations (the comparison with a g2o build is unpinned: g2o needs Eigen):
 *   - the reduced (pose) system is solved by a dense Cholesky without pivoting
 *     in ascending pose order, not Eigen's SimplicialLDLT behind a fill-reducing
 *     ordering; a pivot that is not positive (or NaN) is the failed solve;
 *   - the 3x3 inverse of a point block is restated from cofactors;
 *   - a failed solve is a rejected zero step;
 *   - pbStopFlag is read before the call only (the adapter's business); g2o's
 *     mid-run terminate() is not reproduced;
 *   - the matrix products of the quadratic form are associated as
 *     tests/localba_ref.py writes them.
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error().
 */
#ifndef ORBGPU_LOCALBA_H
#define ORBGPU_LOCALBA_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One job owns ranges of the batch's concatenated arrays.
 *   poses  [pose_offset, pose_offset + n_poses): the n_local local keyframes
 *          first (lLocalKeyFrames order), then the fixed ones (lFixedCameras)
 *       Tcw    float[12]: GetPose(), row-major 3x4 [R|t]
 *       fixed  uint8: the local keyframe with mnId == 0; ignored (taken as set)
 *              for the fixed keyframes
 *       cam    float[5]: the keyframe's fx, fy, cx, cy, mbf
 *   points [point_offset, point_offset + n_points): lLocalMapPoints order
 *       Xw     float[3]: GetWorldPos()
 *   edges  [edge_offset, edge_offset + n_edges): grouped by point, within a
 *          point in GetObservations() order
 *       edge_pose, edge_point  int: indices within the job; edge_point must not
 *              decrease
 *       obs    float[3]: mvKeysUn[i].pt.x, .pt.y, mvuRight[i]; uRight < 0 makes
 *              the monocular edge, otherwise the stereo edge
 *       inv_sigma2  float: mvInvLevelSigma2[octave]
 *   outputs: Tcw_out float[16] for local pose k at out_pose_offset + k, Xw_out
 *   float[3] at the point's index, erase uint8 at the edge's index.
 * Ranges of different jobs must not overlap. */
typedef struct orbgpu_localba_job {
    int n_poses, n_local, n_points, n_edges;
    int pose_offset, point_offset, edge_offset, out_pose_offset;
} orbgpu_localba_job;

typedef struct orbgpu_localba_result {
    int rounds;           /* 0 when n_edges == 0, else 2; -1 for a rejected job             */
    int n_bad_first;      /* edges sent to level 1 after the first round                      */
    int n_erase;          /* edges flagged by the final test (vToErase.size())               */
    int pad;
    int lm_iterations[2]; /* diagnostics: LM iterations and rejected trials per round; they  */
    int lm_rejected[2];   /* depend on rounding noise at convergence                          */
} orbgpu_localba_result;

/* Bytes of workspace a call needs; it depends on the totals and on max_local,
 * an upper bound of every job's n_local, only.  0 for a negative argument. */
size_t orbgpu_local_ba_workspace_bytes(int batch, int total_poses, int total_points, int total_edges,
                                       int max_local);

/* Batched, HBM-resident (jobs included), asynchronous on `stream`; one
 * workgroup per job, the whole optimisation inside one launch, no
 * synchronisation between workgroups.  d_workspace is scratch of at least
 * orbgpu_local_ba_workspace_bytes(...) bytes, 8-byte aligned, the call's until
 * it has completed.  A job's outputs do not depend on the batch it runs in or
 * on its position, and repeat bit for bit from call to call; bytes outside
 * every job's ranges are not written.
 * ORBGPU_ERR_ARG, checked before the device is: a negative count, a NULL
 * d_jobs / d_results with batch > 0, a NULL array whose total is positive, a
 * NULL or too small workspace with batch > 0.  The jobs live on the device, so
 * a job with a negative count or offset, a range beyond a total, n_local >
 * n_poses or > max_local, an edge index out of range or edge_point decreasing
 * reads nothing else, writes nothing but its result and gets rounds = -1, while
 * the call still returns ORBGPU_OK. */
int orbgpu_local_ba_batch_device(int batch, const orbgpu_localba_job* d_jobs, int total_poses, int total_local,
                                 int total_points, int total_edges, int max_local, const float* d_Tcw,
                                 const uint8_t* d_fixed, const float* d_cam, const float* d_Xw,
                                 const int* d_edge_pose, const int* d_edge_point, const float* d_obs,
                                 const float* d_inv_sigma2, float* d_Tcw_out, float* d_Xw_out, uint8_t* d_erase,
                                 orbgpu_localba_result* d_results, void* d_workspace, size_t workspace_bytes,
                                 void* stream);
/* Host-pointer form (uploads, runs, downloads, synchronises).  d_workspace is
 * device memory as above, or NULL: the call then allocates its own for its
 * duration (workspace_bytes is ignored).  The checks above and, per job, every
 * condition that gives rounds = -1 in the device form are ORBGPU_ERR_ARG before
 * the device is looked at.  batch == 0 succeeds without a device. */
int orbgpu_local_ba_batch(int batch, const orbgpu_localba_job* jobs, int total_poses, int total_local,
                          int total_points, int total_edges, int max_local, const float* Tcw, const uint8_t* fixed,
                          const float* cam, const float* Xw, const int* edge_pose, const int* edge_point,
                          const float* obs, const float* inv_sigma2, float* Tcw_out, float* Xw_out, uint8_t* erase,
                          orbgpu_localba_result* results, void* d_workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
