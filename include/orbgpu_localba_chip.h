/*
 * orbgpu_localba_chip.h -- C ABI of the local bundle adjustment
 * (Optimizer::LocalBundleAdjustment) of ONE keyframe neighbourhood spread over
 * the whole chip, a launch per phase, driven by the calling thread, with g2o's
 * polls of the force-stop flag.  orbgpu_localba.h's batched form gives a job
 * one workgroup inside one asynchronous launch and cannot see the flag; it
 * stays the right tool for a replay of many jobs.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Optimizer::LocalBundleAdjustment         src/Optimizer.cpp:536-885 (the optimisation: :759-847)
 *   setForceStopFlag(pbStopFlag)             src/Optimizer.cpp:611-612
 *   the read between the rounds              src/Optimizer.cpp:764-766
 *   SparseOptimizer::optimize                Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419
 *   and the g2o pieces listed in orbgpu_localba.h.
 * Caller: LocalMapping::Run with &mbAbortBA.  The gather and the write-back are
 * include/orbslam2_amd/LocalBundleAdjuster.h's.
 *
 * What is restated (tests/localba_chip_ref.py): everything orbgpu_localba.h
 * lists -- optimize(iterations_first) with Huber on every edge, the test
 * chi2 > 5.991 | 7.815 || !isDepthPositive() in double that sends an edge to
 * level 1, optimize(iterations_second) without kernels over the level-0 edges
 * with lambda, ni and the stop counter afresh, the same test over all edges for
 * the erase flags, the active set of initializeOptimization(0) per round, an
 * active edge's chi2 being that of the last trial evaluated, accepted or not,
 * a level-1 edge keeping its stale first-round value, the round trip of every
 * local pose through Converter::toSE3Quat -- on the solver of
 * orbgpu_globalba.h, plus the polls.  Polls are counted from 0 in the order
 * they are made:
 *   - the first round's: at the top of every iteration that i < iterations
 *     admits (sparse_optimizer.cpp:376) and after a rejected trial that another
 *     would follow (optimization_algorithm_levenberg.cpp:149);
 *   - the read between the rounds (:764), a read of its own;
 *   - the second round's.
 * A round without an active vertex, or with 0 iterations, makes no poll.  A
 * poll inside a round that sees the flag ends that round (stopped = 1 at the
 * top of an iteration, 2 after a rejected trial, whose step is not applied).
 * When the read between the rounds sees it, rounds = 1: no edge goes to level
 * 1, there is no second round and the final test runs over all edges.  When it
 * does not, the second round runs even after a stopped first one, which is
 * what the reference does with a flag that was cleared again.  An edge whose
 * error was never evaluated has chi2 0: when poll 0 sees the flag only the
 * depth test can flag an edge.
 *
 * Deviations (the comparison with a g2o build is unpinned: g2o needs Eigen):
 *   - the reduced (pose) system is solved by a dense Cholesky without pivoting
 *     in ascending pose order, not Eigen's SimplicialLDLT behind a fill-reducing
 *     ordering; a pivot that is not positive (or NaN) is the failed solve;
 *   - the back-substitution is column oriented (tests/globalba_ref.py); this
 *     is the one difference in arithmetic from orbgpu_localba.h's form;
 *   - the 3x3 inverse of a point block is restated from cofactors;
 *   - a failed solve is a rejected zero step; the edges then hold the errors of
 *     the kept estimate;
 *   - a NaN among the diagonal entries makes computeLambdaInit's maximum NaN
 *     whatever its position;
 *   - the flag is read by the host between launches: a flag set while a trial
 *     is on the device is seen at the next poll, as g2o sees it at its next;
 *   - the matrix products are associated as tests/localba_ref.py writes them.
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error().
 */
#ifndef ORBGPU_LOCALBA_CHIP_H
#define ORBGPU_LOCALBA_CHIP_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One problem in orbgpu_localba.h's array layout, indices from 0:
 *   poses  [0, n_poses): the n_local local keyframes first, then the fixed ones
 *       Tcw float[12], fixed uint8 (honoured for the local ones, taken as set
 *       for the rest), cam float[5]
 *   points [0, n_points): Xw float[3]
 *   edges  [0, n_edges): grouped by point, edge_point must not decrease
 *       edge_pose, edge_point int, obs float[3], inv_sigma2 float
 *   outputs: Tcw_out float[16] per local pose, Xw_out float[3] per point, erase
 *   uint8 per edge. */
typedef struct orbgpu_localba_chip_result {
    int status;                /* 0, or -1: an edge index out of range / edge_point decreasing; nothing else written */
    int rounds;                /* optimize() calls made: 0 when n_edges == 0, 1 when the read between the rounds saw the flag, else 2 */
    int n_bad_first;           /* edges sent to level 1 (0 when rounds < 2)                              */
    int n_erase;               /* edges flagged by the final test                                        */
    int stop_poll;             /* index of the first poll that saw the flag, -1: none                    */
    int polls;                 /* polls made                                                             */
    int lm_iterations[2];      /* per round, orbgpu_ba_result's meanings: LM iterations begun,           */
    int lm_rejected[2];        /* rejected trials,                                                       */
    int stopped[2];            /* 0, 1 flag seen at the top of an iteration, 2 after a rejected trial,   */
    int iterations_applied[2]; /* the iteration count of a flagless round that leaves the same estimates */
    int n_free[2];             /* per round's active set: free local poses with a level-0 edge           */
    int n_active_points[2];    /* and points with one                                                    */
} orbgpu_localba_chip_result;

/* Bytes of workspace a call needs.  The reduced system is dense, (6 n_local +
 * 1) x 6 n_local doubles.  0 for a negative argument, n_local > n_poses or a
 * size that does not fit a size_t. */
size_t orbgpu_local_ba_chip_workspace_bytes(int n_poses, int n_local, int n_points, int n_edges);

/* HBM-resident arrays, synchronous: the calling thread drives both rounds (a
 * launch per phase on `stream`; one stream synchronisation per trial, one at
 * the start, one at the end and one between the rounds, where the host learns
 * the second round's active set) and the call returns when the optimisation
 * has ended: at most (iterations_first + iterations_second) x (1 + 10) passes
 * on any input.  LocalMapping's numbers are 5 and 10.  stop_flag is a byte of
 * host memory (NULL: none).  stop_at_poll = k >= 0 makes poll k and every
 * later one count as set whatever the flag holds (-1: off): passing a recorded
 * run's stop_poll back reproduces that run bit for bit.  result is host
 * memory.  d_workspace is scratch of at least
 * orbgpu_local_ba_chip_workspace_bytes(...) bytes, 8-byte aligned; nothing is
 * allocated per call (the pinned record the kernels report through is the
 * calling thread's, made at its first call and kept).  Outputs repeat bit for
 * bit from call to call.
 * ORBGPU_ERR_ARG, checked before the device is: a negative count or iteration
 * number, n_local > n_poses, stop_at_poll < -1, a NULL array whose count is
 * positive, a NULL result, a NULL, misaligned or too small workspace, a size
 * that does not fit a size_t.  An edge index out of range or a decreasing
 * edge_point is found by a kernel before any other indexes with it: the call
 * returns ORBGPU_OK with status = -1 and writes nothing else. */
int orbgpu_local_ba_chip_device(int n_poses, int n_local, int n_points, int n_edges, const float* d_Tcw,
                                const uint8_t* d_fixed, const float* d_cam, const float* d_Xw,
                                const int* d_edge_pose, const int* d_edge_point, const float* d_obs,
                                const float* d_inv_sigma2, int iterations_first, int iterations_second,
                                const volatile uint8_t* stop_flag, int stop_at_poll, float* d_Tcw_out,
                                float* d_Xw_out, uint8_t* d_erase, orbgpu_localba_chip_result* result,
                                void* d_workspace, size_t workspace_bytes, void* stream);
/* Host-pointer form (uploads, runs, downloads).  d_workspace is device memory
 * as above, or NULL: the call then allocates its own for its duration
 * (workspace_bytes is ignored).  The checks above and every edge index and the
 * order of edge_point are ORBGPU_ERR_ARG before the device is looked at. */
int orbgpu_local_ba_chip(int n_poses, int n_local, int n_points, int n_edges, const float* Tcw, const uint8_t* fixed,
                         const float* cam, const float* Xw, const int* edge_pose, const int* edge_point,
                         const float* obs, const float* inv_sigma2, int iterations_first, int iterations_second,
                         const volatile uint8_t* stop_flag, int stop_at_poll, float* Tcw_out, float* Xw_out,
                         uint8_t* erase, orbgpu_localba_chip_result* result, void* d_workspace,
                         size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
