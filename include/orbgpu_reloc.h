/*
 * orbgpu_reloc.h -- C ABI of Tracking::Relocalization's candidate loop: the
 * PnPsolver set-up for every (lost frame, candidate keyframe) pair that
 * SearchByBoW(KF, F) matched well enough, and the whole
 * `while (nCandidates > 0 && !bMatch)` loop with its verification -- up to
 * three pose optimisations and two projection searches per returned pose --
 * on the device.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Tracking::Relocalization              src/Tracking.cpp:1747-1914
 *     SearchByBoW(pKF, F), nmatches < 15  :1786-1791 (orbgpu_search_by_bow_batch_device, orbgpu_bow.h)
 *     PnPsolver(F, matches); SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)   :1795-1796
 *     while (nCandidates > 0 && !bMatch) for each candidate: iterate(5)          :1808-1829
 *     the verification of a returned pose :1832-1899
 *   PnPsolver::PnPsolver                  src/PnPsolver.cpp:104-148
 *   PnPsolver::SetRansacParameters        src/PnPsolver.cpp:159-195
 *   PnPsolver::iterate                    src/PnPsolver.cpp:203-301
 *
 * The pieces are the library's own: orbgpu_pnp_ransac_batch_device
 * (orbgpu_ransac.h), orbgpu_pose_optimization_batch_device (orbgpu_poseopt.h)
 * and the ORBGPU_PROJ_KEYFRAME variant of
 * orbgpu_search_by_projection_batch_device (orbgpu_proj.h).  What is added is
 * the device-side schedule, the PnP draws on the device and the glue between
 * the stages, with the reference's quirks kept:
 *   - iterate()'s loop condition is `||` (PnPsolver.cpp:224): a call runs
 *     max(mRansacMaxIts - mnIterations, 5) iterations, so a solver's first
 *     call runs to its maximum unless Refine() returns earlier;
 *   - a solver whose call returned a pose without bNoMore stays alive;
 *   - sFound is not updated by the outlier cull after the first optimisation,
 *     and the outliers of the second optimisation are not nulled before the
 *     second search;
 *   - mvbOutlier starts all zero and persists across the verifications of a
 *     query: PoseOptimization writes it only where a MapPoint is present.
 *
 * Random stream: as in orbgpu_loop.h, each query carries the
 * orbgpu_rand_state it starts from and returns the state after exactly the
 * draws the reference consumed (4 per RANSAC iteration).
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error();
 * *_device functions take HBM pointers and are asynchronous on `stream`.
 */
#ifndef ORBGPU_RELOC_H
#define ORBGPU_RELOC_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"
#include "orbgpu_loop.h"
#include "orbgpu_poseopt.h"
#include "orbgpu_proj.h"
#include "orbgpu_ransac.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A lost frame.  target: N, mvKeysUn, mDescriptors (16-byte aligned), mvuRight
 * (NULL = monocular), bounds, intrinsics, mbf, the scale pyramid; Tcw and
 * occupied are the loop's own and ignored. */
typedef struct orbgpu_reloc_frame {
    orbgpu_proj_target target;
    float level_sigma2[16];       /* mvLevelSigma2     */
    float inv_level_sigma2[16];   /* mvInvLevelSigma2  */
} orbgpu_reloc_frame;

/* One (lost frame, candidate keyframe) pair.  The keyframe is entry `kf` of an
 * orbgpu_loop_keyframe table (world positions and validity of its MapPoint
 * slots; slot i = keypoint i = its MapPoint) and of the parallel
 * orbgpu_loop_keyframe_search table (mvKeysUn, MapPoint descriptors and
 * distance ranges). */
typedef struct orbgpu_reloc_candidate {
    int frame, kf;
} orbgpu_reloc_candidate;

/* One Relocalization() call: candidates [first_cand, first_cand + n_cand) of
 * the candidate table, all of the same frame, in vpCandidateKFs order;
 * n_cand <= ORBGPU_LOOP_MAX_CANDIDATES. */
typedef orbgpu_compute_sim3_query orbgpu_reloc_query;

/* SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) (Tracking.cpp:1796) */
#define ORBGPU_RELOC_MIN_MATCHES 15
#define ORBGPU_RELOC_MAX_ITERATIONS 300
#define ORBGPU_RELOC_ITERATIONS_PER_CALL 5

/* Device workspace of orbgpu_reloc_setup_batch_device: per candidate up to
 * match_stride correspondences (mvP3Dw, mvP2D, mvMaxError, mvKeyPointIndices)
 * and the solver's N, mRansacMinInliers and mRansacMaxIts.  The layout is the
 * library's. */
size_t orbgpu_reloc_setup_workspace_bytes(int n_cand, int match_stride);

/* PnPsolver constructors and SetRansacParameters for n_cand candidates.
 * d_match + c*match_stride is SearchByBoW(pKF, F)'s row of candidate c: per
 * frame keypoint the keyframe slot or -1; d_nmatches[c] its return value.
 * Candidates with d_nmatches[c] < ORBGPU_RELOC_MIN_MATCHES get d_n_corr[c] = -1
 * (discarded before a solver exists); otherwise d_n_corr[c] = N, the number of
 * frame keypoints j, ascending, whose slot holds a valid MapPoint. */
int orbgpu_reloc_setup_batch_device(int n_cand, const orbgpu_reloc_candidate* d_cands,
                                    const orbgpu_reloc_frame* d_frames, const orbgpu_loop_keyframe* d_kfs,
                                    const int* d_match, int match_stride, const int* d_nmatches, void* d_workspace,
                                    int* d_n_corr, void* stream);

enum {
    ORBGPU_RELOC_PENDING = 0,     /* more passes needed */
    ORBGPU_RELOC_MATCHED = 1,     /* a candidate's verification ended with nGood >= 50 */
    ORBGPU_RELOC_NO_MATCH = 2,    /* no candidate is live any more */
    ORBGPU_RELOC_CAPACITY = 3     /* the frame or a candidate keyframe exceeds the projection matcher's
                                     capacity (4096 keypoints or match_stride); nothing truncated */
};

typedef struct orbgpu_relocalize_result {
    int status;               /* ORBGPU_RELOC_*                                   */
    int matched;              /* the candidate (0..n_cand-1) that passed, or -1   */
    int round;                /* round of the last iterate() call (-1: none)      */
    int calls;                /* iterate() calls made                             */
    int verifications;        /* poses returned and verified                      */
    int hypotheses;           /* RANSAC iterations run by all candidates          */
    int draws;                /* rand() values consumed (4 per iteration)         */
    /* the last verification (zero / -1 when there was none) */
    int last_cand;            /* its candidate, or -1                             */
    int n_inliers;            /* nInliers of the iterate() call that returned     */
    int refined;              /* 1: mRefinedTcw, 0: mBestTcw at bNoMore           */
    int nadditional[2];       /* the two SearchByProjection returns (-1: not run) */
    int n_good;               /* the last nGood                                   */
    int pad;
    float pnp_Tcw[16];        /* the pose iterate() returned                      */
    float Tcw[16];            /* mCurrentFrame.mTcw at the end of the verification */
    orbgpu_poseopt_result opt[3];  /* the three PoseOptimization calls (unused: zero, rounds = 0) */
    orbgpu_rand_state rng_after;   /* stream state after exactly the consumed draws */
} orbgpu_relocalize_result;

/* Per candidate after the last pass: the solver's state. */
typedef struct orbgpu_reloc_candidate_state {
    int n;                    /* N correspondences (-1: discarded before a solver existed) */
    int min_inliers;          /* mRansacMinInliers after SetRansacParameters     */
    int max_iterations;       /* mRansacMaxIts after SetRansacParameters         */
    int iterations;           /* mnIterations                                    */
    int best_inliers;         /* mnBestInliers                                   */
    int discarded;            /* vbDiscarded                                     */
} orbgpu_reloc_candidate_state;

#define ORBGPU_RELOC_ROWS 5

/* Bytes of the opaque device state block of orbgpu_relocalize_batch_device. */
size_t orbgpu_relocalize_workspace_bytes(int n_queries, int n_cand, int match_stride);

/* The reference's loop for every query, one workgroup per query in every
 * stage.  One *pass* takes every unfinished query through one iterate(5) call
 * of its next live candidate (calls that draw nothing -- N < mRansacMinInliers
 * -- are made on the way) and, when the call returns a pose, through the whole
 * verification; n_passes >= 1 passes are enqueued on `stream` with no host
 * synchronisation, and a pass does nothing for a finished query.  resume = 0
 * starts every query from its rng; resume = 1 continues from d_state as an
 * earlier call with the same arguments left it.  A query's result, candidate
 * states and rows do not depend on how the passes are split over calls or on
 * the batch it runs in.
 *   d_kf_search      table parallel to d_kfs
 *   d_match          SearchByBoW's rows as for orbgpu_reloc_setup_batch_device;
 *                    d_setup: the workspace that call filled
 *   d_cand_states    per candidate, the solver state after the last pass
 *   d_rows           int[n_queries][ORBGPU_RELOC_ROWS][match_stride], by frame
 *                    keypoint, of the last verification: vbInliers (0/1);
 *                    mvpMapPoints (keyframe slot or -1) after the first
 *                    optimisation and its outlier cull, after the second
 *                    optimisation, and at the end of the verification (stages
 *                    that did not run repeat the row before); mvbOutlier (0/1),
 *                    which persists across the verifications of a query
 * ORBGPU_ERR_ARG comes before the device is looked at; n_queries == 0 needs
 * no device. */
int orbgpu_relocalize_batch_device(int n_queries, const orbgpu_reloc_query* d_queries, int n_cand,
                                   const orbgpu_reloc_candidate* d_cands, const orbgpu_reloc_frame* d_frames,
                                   const orbgpu_loop_keyframe* d_kfs, const orbgpu_loop_keyframe_search* d_kf_search,
                                   const int* d_match, int match_stride, const void* d_setup, int n_passes,
                                   int resume, void* d_state, orbgpu_relocalize_result* d_results,
                                   orbgpu_reloc_candidate_state* d_cand_states, int* d_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
