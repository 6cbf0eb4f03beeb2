/*
 * orbgpu_track.h -- C ABI of Tracking's per-frame chain on the device: the
 * initial pose estimate (TrackWithMotionModel / TrackReferenceKeyFrame), the
 * local-map refinement (SearchLocalPoints + TrackLocalMap) and the stereo /
 * RGB-D visual-odometry points of UpdateLastFrame.  Each entry point is
 * batched over independent frames (several cameras, or a replay), enqueues
 * all its stages on `stream` and synchronises with the host nowhere.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Tracking::TrackReferenceKeyFrame      src/Tracking.cpp:977-1025
 *   Tracking::UpdateLastFrame             src/Tracking.cpp:1033-1114
 *   Tracking::TrackWithMotionModel        src/Tracking.cpp:1126-1198
 *   Tracking::TrackLocalMap               src/Tracking.cpp:1210-1264
 *   Tracking::SearchLocalPoints           src/Tracking.cpp:1496-1562
 *   Frame::UnprojectStereo                src/Frame.cpp:780-796
 *
 * The pieces are the library's own: the ORBGPU_PROJ_LAST_FRAME and
 * ORBGPU_PROJ_LOCAL variants of orbgpu_search_by_projection_batch_device
 * (orbgpu_proj.h), orbgpu_pose_optimization_batch_device (orbgpu_poseopt.h)
 * and, for the reference-keyframe mode, the row of
 * orbgpu_search_by_bow_batch_device (orbgpu_bow.h).  What is added is the glue
 * between them, one workgroup per frame, and a batched Frame::isInFrustum that
 * reads its pose from HBM.  A frame that is not in a stage hands that stage an
 * empty job (n = 0) or an idle call.
 *
 * UpdateLocalMap (Tracking.cpp:1217) sits between the two halves and depends on
 * the first half's matches, so the chain is two entry points here.  The caller
 * either runs it on the host, or calls orbgpu_update_local_map_batch_device
 * (orbgpu_localmap.h) between the two on the same stream: it reads call 1's
 * rows in place and writes call 2's table, frame_mp and job.  The MapPoint
 * counters (IncreaseVisible, IncreaseFound), mbTrackInView / mnLastFrameSeen
 * and the fallback from the motion model to the reference keyframe stay with
 * the caller, who re-submits a FEW_MATCHES or LOST frame in reference mode as
 * Track() does.
 *
 * Quirks of the reference that are kept:
 *   - the 2*th retry starts from an all-NULL mvpMapPoints (:1158), so a match
 *     of the first search never hides a keypoint from the second;
 *   - only row entries >= 0 become mvpMapPoints: the -2 entries of a
 *     LAST_FRAME call are that call's own assignments, culled by its rotation
 *     check (ORBmatcher.cpp:1616-1630), on a row that was NULL before it;
 *   - nmatches is decremented by the cull, nmatchesMap counts only the kept
 *     points with Observations() > 0 (:1172-1189, :1005-1022);
 *   - with mbOnlyTracking the return is nmatches > 20 (strictly) while the
 *     search threshold is nmatches < 20 (:1156, :1162, :1194);
 *   - TrackReferenceKeyFrame does not look at isBad() after SearchByBoW: the
 *     row itself is mvpMapPoints (:996);
 *   - SearchLocalPoints nulls a held bad point but marks every other held
 *     point seen, whether it has observations or not (:1501-1520);
 *   - a point call 1 culled has mnLastFrameSeen == mnId (:1016, :1183) and is
 *     skipped by SearchLocalPoints (:1531) like a held one, without being held:
 *     ORBGPU_PT_LAST_SEEN in call 2's table;
 *   - SearchByProjection(F, vpMapPoints) may reassign a keypoint that holds a
 *     point without observations and never one with (ORBmatcher.cpp:113);
 *   - TrackLocalMap nulls the outliers only with mSensor == STEREO (:1248),
 *     and an RGB-D stream keeps them;
 *   - mnMatchesInliers counts every non-outlier with mbOnlyTracking and only
 *     those with Observations() > 0 without (:1238-1246);
 *   - UpdateLastFrame increments nPoints in both branches (:1104, :1108), so
 *     the loop's exit depends on the visited, not the created, points.
 *
 * mvbOutlier needs no row after orbgpu_track_initial_batch_device: the cull
 * resets the flag where it nulls a point (:1014, :1181), so afterwards it is
 * false wherever the frame holds a point.
 *
 * Conventions as in orbgpu.h: int status returns, orbgpu_last_error();
 * *_device functions take HBM pointers and are asynchronous on `stream`.
 * Argument errors are ORBGPU_ERR_ARG before the device is looked at; n == 0
 * needs no device.  A frame's result and rows do not depend on the batch it
 * runs in or on its position, and repeat bit for bit.
 */
#ifndef ORBGPU_TRACK_H
#define ORBGPU_TRACK_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu.h"
#include "orbgpu_poseopt.h"
#include "orbgpu_proj.h"
#include "orbgpu_reloc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    ORBGPU_TRACK_MOTION = 0,     /* TrackWithMotionModel   */
    ORBGPU_TRACK_REFERENCE = 1   /* TrackReferenceKeyFrame */
};

enum {
    ORBGPU_TRACK_OK = 0,          /* the reference returns true                                    */
    ORBGPU_TRACK_FEW_MATCHES = 1, /* false before the optimisation (:992, :1162); Tcw = the start  */
    ORBGPU_TRACK_LOST = 2,        /* false after the optimisation                                  */
    ORBGPU_TRACK_CAPACITY = 3,    /* the frame has more keypoints than `stride` or 4096, or (local
                                     map) more points than `point_stride`; nothing truncated       */
    ORBGPU_TRACK_BAD_JOB = 4      /* mode or frame out of range, points.n < 0, n_local < 0 or
                                     > points.n, a NULL bow_row / bow_nmatches (reference mode),
                                     Tcw or frame_mp; nothing but the job's own result and rows
                                     is touched                                                    */
};

#define ORBGPU_TRACK_MIN_MATCHES 20      /* :1156, :1162 */
#define ORBGPU_TRACK_MIN_BOW_MATCHES 15  /* :992         */
#define ORBGPU_TRACK_MIN_MAP_MATCHES 10  /* :1024, :1193, :1197 */

/* ---- 1. TrackWithMotionModel / TrackReferenceKeyFrame ---------------------
 * The frame table is orbgpu_reloc_frame's (target plus the two sigma tables);
 * target.Tcw and target.occupied are ignored: the frame's occupancy is all
 * NULL (:1141) and its pose is the job's.
 *
 * Motion mode.  points is indexed by the LAST frame's keypoint slot i:
 * flags ORBGPU_PT_VALID = mvpMapPoints[i] && !mvbOutlier[i], ORBGPU_PT_HAS_OBS;
 * pos, desc, octave (mvKeys[i].octave) and angle.  Tcw_init is the caller's
 * mVelocity * mLastFrame.mTcw (:1139), last_Tcw = mLastFrame.mTcw.  th is 15,
 * or 7 for a stereo stream (:1145-1148); mono = (mSensor == MONOCULAR).
 * ORBmatcher(0.9, true).
 *
 * Reference mode.  points is indexed by the reference keyframe's slot: flags
 * (VALID = pMP && !pMP->isBad() as SearchByBoW saw it, HAS_OBS) and pos.
 * bow_row / bow_nmatches: device pointers to SearchByBoW(refKF, F)'s row (per
 * frame keypoint the keyframe slot or -1) and return value.  Tcw_init is
 * mLastFrame.mTcw (:997); last_Tcw, th and mono are not read. */
typedef struct orbgpu_track_initial_job {
    int mode;                 /* ORBGPU_TRACK_MOTION / _REFERENCE */
    int frame;                /* index into the frame table       */
    int mono;
    int only_tracking;        /* mbOnlyTracking                   */
    float th;
    int pad[3];
    float Tcw_init[16];
    float last_Tcw[16];
    orbgpu_proj_points points;
    const int* bow_row;
    const int* bow_nmatches;
} orbgpu_track_initial_job;

typedef struct orbgpu_track_initial_result {
    int status;               /* ORBGPU_TRACK_*                                            */
    int searches;             /* SearchByProjection calls made (0, 1 or 2)                 */
    int nsearch[2];           /* their return values (-1: not run)                         */
    int nmatches;             /* after the cull (before it when no optimisation ran; the
                                 BoW return in reference mode)                             */
    int nmatches_map;         /* nmatchesMap                                               */
    int vo;                   /* mbVO (only_tracking, motion mode), else 0                 */
    int pad;
    orbgpu_poseopt_result opt; /* zero when no optimisation ran                            */
    float Tcw[16];            /* mCurrentFrame.mTcw at the end: Tcw_init when no
                                 optimisation ran (zero for CAPACITY / BAD_JOB)            */
} orbgpu_track_initial_result;

#define ORBGPU_TRACK_INITIAL_ROWS 2

size_t orbgpu_track_initial_workspace_bytes(int n, int stride);

/* d_rows: int[n][2][stride] by frame keypoint: mvpMapPoints (the index into the
 * job's point table, or -1) before the cull and after it; the difference is
 * the set of points whose mbTrackInView / mnLastFrameSeen the host updates.
 * Both rows are all -1 for a frame without an optimisation. */
int orbgpu_track_initial_batch_device(int n, const orbgpu_track_initial_job* d_jobs, int n_frames,
                                      const orbgpu_reloc_frame* d_frames, int stride, void* d_workspace,
                                      orbgpu_track_initial_result* d_results, int* d_rows, void* stream);

/* ---- 2. SearchLocalPoints + TrackLocalMap ---------------------------------
 * The point table: entries [0, n_local) are mvpLocalMapPoints in order; the
 * points the frame holds that are not among them (the stereo visual-odometry
 * points) follow.  flags VALID = !isBad(), HAS_OBS, and ORBGPU_PT_LAST_SEEN =
 * (pMP->mnLastFrameSeen == mCurrentFrame.mnId) before the call, which is how
 * the two calls meet: the cull of call 1 sets mnLastFrameSeen on every point it
 * nulls (:1016, :1183), so SearchLocalPoints skips it at :1531 -- it is not
 * projected, not counted in nToMatch, gets no IncreaseVisible and cannot be
 * matched again in this frame, although the frame no longer holds it.  The
 * caller sets the flag on the entries of the points in row 0 and not in row 1
 * of call 1 (held points are seen through frame_mp and need no flag); pos,
 * normal, desc, min_dist, max_dist.  frame_mp: per frame keypoint an index into the table or
 * -1 -- mvpMapPoints as call 1 and the host left it.  Tcw: a device pointer to
 * 16 floats read when the call runs, so it can name &d_results[k].Tcw of
 * orbgpu_track_initial_batch_device in place.  th is 1, 3 (RGB-D) or 5
 * (recently relocalised) (:1550-1557); ORBmatcher(0.8). */
typedef struct orbgpu_track_local_job {
    int frame;
    int n_local;
    int stereo;               /* mSensor == STEREO                               */
    int only_tracking;
    int recently_relocalised; /* mnId < mnLastRelocFrameId + mMaxFrames (:1257)  */
    float th;
    const float* Tcw;
    const int* frame_mp;
    orbgpu_proj_points points;
} orbgpu_track_local_job;

typedef struct orbgpu_track_local_result {
    int status;               /* OK, LOST, CAPACITY, BAD_JOB                     */
    int n_to_match;           /* nToMatch (:1526-1545)                           */
    int nsearch;              /* SearchByProjection's return (-1: not run)       */
    int n_inliers;            /* mnMatchesInliers                                */
    orbgpu_poseopt_result opt;
    float Tcw[16];
} orbgpu_track_local_result;

#define ORBGPU_PT_LAST_SEEN 8       /* call 2's table flags: mnLastFrameSeen == mnId before the call */
#define ORBGPU_TRACK_LOCAL_ROWS 3
#define ORBGPU_TRACK_PT_SEEN 1     /* d_point_flags: held by the frame and good: IncreaseVisible (:1513-1516) */
#define ORBGPU_TRACK_PT_IN_VIEW 2  /* d_point_flags: isInFrustum passed (IncreaseVisible, :1539)       */

size_t orbgpu_track_local_workspace_bytes(int n, int stride, int point_stride);

/* d_rows: int[n][3][stride] by frame keypoint: mvpMapPoints after
 * SearchLocalPoints, the final mvpMapPoints, mvbOutlier (0 / 1).
 * d_point_flags: uint8[n][point_stride], one byte per table entry. */
int orbgpu_track_local_map_batch_device(int n, const orbgpu_track_local_job* d_jobs, int n_frames,
                                        const orbgpu_reloc_frame* d_frames, int stride, int point_stride,
                                        void* d_workspace, orbgpu_track_local_result* d_results, int* d_rows,
                                        uint8_t* d_point_flags, void* stream);

/* ---- 3. UpdateLastFrame's visual-odometry points (:1053-1113) -------------
 * For stereo and RGB-D streams: what fills call 1's point table for the slots
 * without a MapPoint.  Precondition: a held slot (ORBGPU_PT_VALID) is not an
 * outlier -- Track() nulls those before it copies the frame (:578-584, :601).
 * The slots with z > 0 are ordered by (z, i) (std::sort of pair<float,int>,
 * :1069); the loop visits them in that order, creates a point where the slot
 * holds none or one without observations, and stops after the first visited j
 * with z_j > th_depth and more than 100 visited.  Both branches count, so the
 * visited set is the first min(n_pos, max(m, 100) + 1) of the order, m = the
 * depths in (0, th_depth]; the kernel selects by rank instead of sorting.
 * A created slot gets VALID set and HAS_OBS cleared, pos =
 * Frame::UnprojectStereo(i) (mRwc * x3Dc in double rounded to float, + mOw) and
 * desc = the frame's own descriptor row (the MapPoint(x3D, pMap, pFrame, idx)
 * constructor).  frame_desc and desc are read and written 16 bytes at a time:
 * their device addresses must be 16-byte aligned (hipMalloc's are). */
typedef struct orbgpu_update_last_frame_job {
    int n;                    /* mLastFrame.N (<= stride and 4096) */
    float th_depth;           /* mThDepth                          */
    const float* depth;       /* mvDepth                           */
    const orbgpu_keypoint* kps_un; /* mvKeysUn                     */
    const uint8_t* frame_desc; /* mDescriptors, n x 32             */
    float fx, fy, cx, cy, invfx, invfy;
    float Rwc[9];             /* mRwc, row-major                   */
    float Ow[3];              /* mOw                               */
    int* flags;               /* the slot table, read and written  */
    float* pos;
    uint8_t* desc;
} orbgpu_update_last_frame_job;

typedef struct orbgpu_update_last_frame_result {
    int status;               /* OK, CAPACITY (n > stride or 4096: nothing written but
                                 this result and the frame's zero d_created row) */
    int n_created;
    int n_pos;                /* slots with z > 0      */
    int n_visited;            /* slots the loop visits */
} orbgpu_update_last_frame_result;

/* d_created: uint8[n][stride], 1 where a point was created. */
int orbgpu_update_last_frame_batch_device(int n, const orbgpu_update_last_frame_job* d_jobs, int stride,
                                          orbgpu_update_last_frame_result* d_results, uint8_t* d_created,
                                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
