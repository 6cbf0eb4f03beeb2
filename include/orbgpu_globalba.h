/*
 * orbgpu_globalba.h -- C ABI of the global bundle adjustment
 * (Optimizer::BundleAdjustment / GlobalBundleAdjustemnt): one problem per call
 * -- every keyframe pose and every MapPoint of a map against every observation
 * -- spread over the whole chip, a launch per phase.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Optimizer::BundleAdjustment              src/Optimizer.cpp:72-269 (the optimisation: :218-219)
 *   SparseOptimizer::optimize                Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419
 *   and the g2o pieces listed in orbgpu_localba.h.
 * Callers: Tracking::CreateInitialMapMonocular (src/Tracking.cpp:887: 20
 * iterations, robust) and LoopClosing::RunGlobalBundleAdjustment
 * (src/LoopClosing.cpp:782: 10 iterations, &mbStopGBA, not robust).  The gather
 * and the write-back are include/orbslam2_amd/BundleAdjuster.h's.
 *
 * What is restated: one optimize(n_iterations) with every edge at level 0;
 * Huber on every edge iff `robust`, delta = (float)sqrt(5.99) for a monocular
 * edge (:112: 5.99, not LocalBA's 5.991) and (float)sqrt(7.815) for a stereo
 * edge; edges, Jacobians, quadratic form, Schur complement, the 3x3 inverse
 * from cofactors, lambda on every diagonal, computeLambdaInit, computeScale
 * over poses then points and oplus as orbgpu_localba.h lists them.  The active
 * set is initializeOptimization(0)'s: a pose or point that no edge touches is
 * not optimised, not damped and not in the lambda maximum, a free pose without
 * edges has no rows in the reduced system, and with no active vertex
 * optimize() does nothing.  Every pose is written as Converter::toCvMat(SE3Quat)
 * of its estimate after Converter::toSE3Quat, so a fixed or untouched pose does
 * not in general keep its input bits; a point without edges keeps its bits.
 * n_iterations == 0 and n_edges == 0 run nothing and write that round trip.
 * The force-stop flag is polled where g2o polls it, by the host loop: at the
 * top of every iteration (sparse_optimizer.cpp:376) and after a rejected trial
 * that another would follow (optimization_algorithm_levenberg.cpp:149).
 *
 * Deviations (the comparison with a g2o build is unpinned: g2o needs Eigen):
 *   - the reduced (pose) system is solved by a dense Cholesky without pivoting
 *     in ascending pose order, not Eigen's sparse solver; a pivot that is not
 *     positive (or NaN) is the failed solve;
 *   - a failed solve is a rejected zero step;
 *   - the back-substitution is column oriented (tests/globalba_ref.py);
 *   - a NaN among the diagonal entries makes computeLambdaInit's maximum NaN
 *     whatever its position;
 *   - the matrix products are associated as tests/globalba_ref.py writes them.
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error().
 */
#ifndef ORBGPU_GLOBALBA_H
#define ORBGPU_GLOBALBA_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arrays, in orbgpu_localba.h's layout:
 *   poses  [0, n_poses): every pose is an output pose
 *       Tcw    float[12]: GetPose(), row-major 3x4 [R|t]
 *       fixed  uint8: honoured for every pose (the adapter sets it for mnId == 0)
 *       cam    float[5]: fx, fy, cx, cy, mbf
 *   points [0, n_points)
 *       Xw     float[3]: GetWorldPos()
 *   edges  [0, n_edges): grouped by point, edge_point must not decrease
 *       edge_pose, edge_point  int
 *       obs    float[3]: x, y, uRight; uRight < 0 makes the monocular edge
 *       inv_sigma2  float
 *   outputs: Tcw_out float[16] per pose, Xw_out float[3] per point. */
typedef struct orbgpu_ba_result {
    int status;             /* 0, or -1 for a rejected problem (an edge index out of range or edge_point decreasing) */
    int iterations;         /* LM iterations begun                                                   */
    int rejected;           /* rejected trials                                                       */
    int stopped;            /* 0 ran to its end, 1 flag seen at the top of an iteration, 2 after a rejected trial */
    int iterations_applied; /* the n_iterations of a flagless run that leaves the same estimates     */
    int n_free;             /* free poses with an edge: the reduced system has 6 n_free unknowns     */
    int n_active_points;    /* points with an edge                                                   */
    int pad;
    double first_chi2;      /* robust chi2 at the inputs (0 when no iteration began)                 */
    double last_chi2;       /* robust chi2 of the estimates written                                  */
    double last_lambda;
} orbgpu_ba_result;

/* Bytes of workspace a call needs.  The reduced system is dense, (6 n_poses +
 * 1) x 6 n_poses doubles: capacity is the caller's memory.  0 for a negative
 * argument or when the size does not fit a size_t. */
size_t orbgpu_bundle_adjustment_workspace_bytes(int n_poses, int n_points, int n_edges);

/* HBM-resident arrays, one problem, synchronous: the calling thread drives the
 * LM loop (a launch per phase on `stream`, one stream synchronisation per
 * trial) and the call returns when the optimisation has ended; at most
 * n_iterations x (1 + 10) passes on any input.  stop_flag is host memory (NULL:
 * never stops).  result is host memory.  d_workspace is scratch of at least
 * orbgpu_bundle_adjustment_workspace_bytes(...) bytes, 8-byte aligned; nothing
 * is allocated per call (the pinned record the kernels report through is the
 * calling thread's, made at its first call and kept).  Outputs repeat bit for
 * bit from call to call.
 * ORBGPU_ERR_ARG, checked before the device is: a negative count or
 * n_iterations, a NULL array whose count is positive, a NULL result, a NULL,
 * misaligned or too small workspace.  An edge index out of range or a
 * decreasing edge_point is found by a kernel before any other indexes with
 * it: the call returns ORBGPU_OK with status = -1 and writes nothing else. */
int orbgpu_bundle_adjustment_device(int n_poses, int n_points, int n_edges, const float* d_Tcw, const uint8_t* d_fixed,
                                    const float* d_cam, const float* d_Xw, const int* d_edge_pose,
                                    const int* d_edge_point, const float* d_obs, const float* d_inv_sigma2,
                                    int n_iterations, int robust, const volatile uint8_t* stop_flag, float* d_Tcw_out,
                                    float* d_Xw_out, orbgpu_ba_result* result, void* d_workspace,
                                    size_t workspace_bytes, void* stream);
/* Host-pointer form (uploads, runs, downloads).  d_workspace is device memory
 * as above, or NULL: the call then allocates its own for its duration
 * (workspace_bytes is ignored).  The checks above and every edge index and the
 * order of edge_point are ORBGPU_ERR_ARG before the device is looked at. */
int orbgpu_bundle_adjustment(int n_poses, int n_points, int n_edges, const float* Tcw, const uint8_t* fixed,
                             const float* cam, const float* Xw, const int* edge_pose, const int* edge_point,
                             const float* obs, const float* inv_sigma2, int n_iterations, int robust,
                             const volatile uint8_t* stop_flag, float* Tcw_out, float* Xw_out,
                             orbgpu_ba_result* result, void* d_workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
