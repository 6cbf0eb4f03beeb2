/*
 * orbgpu_localmap.h -- C ABI of Tracking::UpdateLocalMap on the device: the step
 * between the two halves of orbgpu_track.h.  It reads the rows
 * orbgpu_track_initial_batch_device left in HBM and a mirror of the map, and
 * writes the point table, frame_mp and the orbgpu_track_local_job that
 * orbgpu_track_local_map_batch_device reads, so an ordinary frame is three calls
 * on one stream with nothing downloaded, built or uploaded between them.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   Tracking::UpdateLocalMap         src/Tracking.cpp:1571-1581
 *   Tracking::UpdateLocalPoints      src/Tracking.cpp:1588-1615
 *   Tracking::UpdateLocalKeyFrames   src/Tracking.cpp:1622-1745
 *
 * Quirks of the reference that are kept:
 *   - a held bad point is nulled in mCurrentFrame.mvpMapPoints (:1641) and does
 *     not vote; a point held at two keypoints votes twice (:1627-1637);
 *   - with an empty keyframeCounter the function returns (:1646):
 *     mvpLocalKeyFrames and mpReferenceKF keep their previous values and
 *     UpdateLocalPoints runs on the previous list (status KEPT);
 *   - K1 is every voted keyframe that is not bad, in std::map<KeyFrame*,int>
 *     order; pKFmax is the first strict maximum in that order among the non-bad
 *     only (:1660-1676).  With every voted keyframe bad the list is empty, the
 *     reference keyframe is unchanged (ref_kf = -1) and there are no local points;
 *   - the K2 loop visits the K1 members only (itEndKF is taken before anything
 *     is appended, :1682) and stops at the top of an iteration once the list
 *     holds more than 80 (:1685);
 *   - each visited keyframe adds at most one neighbour: the first of its best 10
 *     covisibles that is not bad and not yet marked, then `break` (:1691-1705).
 *     An eleventh covisible is never looked at;
 *   - and at most one child: the first in GetChilds()' std::set order that is
 *     not bad and not marked (:1708-1721);
 *   - pParent is NOT tested for isBad(), and when an unmarked parent is appended
 *     the `break` at :1732 leaves the OUTER loop: the whole K2 walk ends there;
 *   - UpdateLocalPoints walks the keyframes in list order and the slots
 *     ascending, skips NULL slots, points already marked and bad points; the
 *     first occurrence of a point decides its position (:1594-1614);
 *   - the mnTrackReferenceForFrame marks are compared with the current frame's
 *     id only, so marks that are fresh for every job are equivalent.
 *
 * Order.  The reference's std::map<KeyFrame*,int> and std::set<KeyFrame*> iterate
 * in heap-address order, which is not reproducible from run to run even in the
 * reference.  Here the order is the caller's: kf_by_rank lists the keyframe
 * indices in the order that stands for the std::map's (NULL = ascending index; it
 * must be a permutation of 0..n_kf-1), and each keyframe's child list is given in
 * the order that stands for the std::set's.  Only the range of kf_by_rank's
 * entries is checked: one that names a keyframe twice or leaves one out gives a
 * wrong result (a keyframe twice in K1, or a voted frame taken for KEPT), not
 * BAD_JOB.
 *
 * Conventions as in orbgpu.h and orbgpu_track.h.  Everything is integers and
 * copied bytes: a job's outputs are a function of the job and the mirror alone,
 * whatever the batch, the job's position or the run.
 */
#ifndef ORBGPU_LOCALMAP_H
#define ORBGPU_LOCALMAP_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu_track.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the map mirror --------------------------------------------------------
 * A host struct of device pointers to plain arrays.  The caller owns them and
 * keeps them current (LocalMapping changes the map at keyframe rate); many jobs
 * and many calls may share one mirror.  Nothing here is written by the library.
 *
 * Keyframes 0..n_kf-1:
 *   kf_bad        isBad()
 *   slot_offset / n_slots   GetMapPointMatches(): slots[slot_offset[k] + s], a
 *                 point id or -1 for NULL
 *   covis         10 ints per keyframe: the first 10 of
 *                 mvpOrderedConnectedKeyFrames, padded with -1
 *   child_offset / n_children   GetChilds() into children[]
 *   parent        GetParent(), -1 for none
 *   kf_by_rank    optional, see "Order" above
 * Points 0..n_pt-1:
 *   pt_flags      ORBGPU_PT_VALID = !isBad(), ORBGPU_PT_HAS_OBS
 *   obs_offset / n_obs   GetObservations() into obs[] (keyframe indices)
 *   pos, normal (3 floats), desc (32 bytes, the array 16-byte aligned),
 *   min_dist, max_dist: orbgpu_track_local_job's convention, the members
 *   themselves (the /0.8f and /1.2f of GetMin/MaxDistanceInvariance undone). */
typedef struct orbgpu_map_mirror {
    int n_kf, n_pt;
    int n_slots_total, n_children_total, n_obs_total; /* lengths of slots[], children[], obs[] */
    int pad;
    const uint8_t* kf_bad;
    const int* slot_offset;
    const int* n_slots;
    const int* slots;
    const int* covis;
    const int* child_offset;
    const int* n_children;
    const int* children;
    const int* parent;
    const int* kf_by_rank;
    const int* pt_flags;
    const int* obs_offset;
    const int* n_obs;
    const int* obs;
    const float* pos;
    const float* normal;
    const uint8_t* desc;
    const float* min_dist;
    const float* max_dist;
} orbgpu_map_mirror;

#define ORBGPU_LOCALMAP_COVIS 10       /* GetBestCovisibilityKeyFrames(10) (:1691) */
#define ORBGPU_LOCALMAP_MAX_KFS 80     /* :1685                                    */

enum {
    ORBGPU_LOCALMAP_OK = 0,
    ORBGPU_LOCALMAP_KEPT = 1,     /* no votes (:1646): the previous list was used, ref_kf = -1       */
    ORBGPU_LOCALMAP_CAPACITY = 2, /* see below                                                       */
    ORBGPU_LOCALMAP_BAD_JOB = 3   /* an id the job reads lies outside the mirror (a row entry beyond
                                     src_n, a src_pt_id, a slot, an observation, a covis, a child, a
                                     parent, a previous keyframe, a kf_by_rank entry, or an offset +
                                     count beyond its array), or a NULL pointer it needs.  Nothing but
                                     the job's own result is written, and the prepared job gets
                                     frame = -1, so call 2 reports ORBGPU_TRACK_BAD_JOB              */
};

/* One frame.  rows is call 1's d_rows + k * 2 * stride, read in place: row 0
 * (before the cull) at [0, stride), row 1 (after it, the frame's mvpMapPoints)
 * at [stride, 2 * stride); both index call 1's point table of src_n entries.
 * src_pt_id: per entry of that table the mirror's point id, or -1 for a temporal
 * visual-odometry point (UpdateLastFrame's), whose pos and desc are then taken
 * from src_pos / src_desc (call 1's table; src_desc 16-byte aligned).
 * prev_kfs / n_prev_kfs: mvpLocalKeyFrames before the call, read only on the
 * empty-vote path.
 *
 * The out_* buffers hold point_stride entries each (out_desc 16-byte aligned),
 * frame_mp `stride` ints.  local_job is the orbgpu_track_local_job of the
 * following call, on the device; its n_local, points.n, points.flags, pos,
 * normal, desc, min_dist, max_dist and frame_mp are written here, everything
 * else (frame, Tcw, th, the mode flags, points.octave ..) is the caller's and is
 * left as it is.
 *
 * The filled table: entries [0, n_local) are mvpLocalMapPoints gathered from
 * the mirror, flags = VALID | the mirror's HAS_OBS | ORBGPU_PT_LAST_SEEN on a
 * point that is in row 0 and not in row 1 of call 1.  The points the frame holds
 * that are not local follow in keypoint order, once each (a point held at two
 * keypoints gets one entry and both frame_mp entries name it): one with a
 * mirror id is gathered from the mirror like a local point, one with id -1 is
 * VALID without HAS_OBS, pos and desc from call 1's table, normal and distances
 * zero (SearchLocalPoints never projects a held point).  frame_mp: per keypoint
 * the table index or -1; held bad points are already nulled; entries from n_kp
 * to stride are -1.
 *
 * CAPACITY.  (a) The local points plus the extras exceed point_stride: every
 * count in the result is the true one, the table and local_points are written up
 * to point_stride, and the prepared job gets the true points.n, so call 2
 * reports ORBGPU_TRACK_CAPACITY by itself.  (b) n_kp exceeds stride or 4096, or
 * the local keyframes exceed kf_stride: the job ends there.  n_local_kfs is the
 * true count and local_kfs holds the first kf_stride; no point is gathered
 * (n_local = n_extra = 0), frame_mp is all -1 and the prepared job gets n_local
 * = 0 and points.n = point_stride + 1, which call 2 reports as CAPACITY too.
 * Nothing is ever written beyond a buffer's capacity. */
typedef struct orbgpu_update_local_map_job {
    int n_kp;                 /* mCurrentFrame.N                              */
    int src_n;                /* entries of call 1's point table              */
    int n_prev_kfs;
    int pad;
    const int* rows;
    const int* src_pt_id;
    const float* src_pos;
    const uint8_t* src_desc;
    const int* prev_kfs;
    int* out_flags;
    float* out_pos;
    float* out_normal;
    uint8_t* out_desc;
    float* out_min_dist;
    float* out_max_dist;
    int* frame_mp;
    orbgpu_track_local_job* local_job;
} orbgpu_update_local_map_job;

typedef struct orbgpu_update_local_map_result {
    int status;               /* ORBGPU_LOCALMAP_*                                        */
    int n_k1;                 /* the voted keyframes that are not bad                     */
    int n_local_kfs;          /* mvpLocalKeyFrames.size()                                 */
    int ref_kf;               /* pKFmax, -1 = mpReferenceKF unchanged                     */
    int n_nulled;             /* held bad points nulled (:1641), counted per keypoint     */
    int n_local;              /* mvpLocalMapPoints.size()                                 */
    int n_extra;              /* held points that are not local                           */
    int pad;
} orbgpu_update_local_map_result;

size_t orbgpu_update_local_map_workspace_bytes(int n, int stride, int point_stride, int kf_stride, int n_kf,
                                               int n_pt);

/* d_local_kfs: int[n][kf_stride], mvpLocalKeyFrames; d_local_points:
 * int[n][point_stride], the mirror ids of mvpLocalMapPoints in order (for
 * SetReferenceMapPoints and the replay of the counters).  Entries past the
 * counts are not written.  `mirror` is a host struct; d_workspace need not be
 * zeroed.  Asynchronous on `stream`: several launches, no host
 * synchronisation, and none between workgroups inside a launch. */
int orbgpu_update_local_map_batch_device(int n, const orbgpu_update_local_map_job* d_jobs,
                                         const orbgpu_map_mirror* mirror, int stride, int point_stride,
                                         int kf_stride, void* d_workspace,
                                         orbgpu_update_local_map_result* d_results, int* d_local_kfs,
                                         int* d_local_points, void* stream);

#ifdef __cplusplus
}
#endif
#endif
