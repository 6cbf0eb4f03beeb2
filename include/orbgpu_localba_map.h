/*
 * orbgpu_localba_map.h -- C ABI of the two host stretches of
 * Optimizer::LocalBundleAdjustment on the device, against the map mirror of
 * orbgpu_localmap.h: the gather that builds orbgpu_localba.h's arrays from the
 * map, and the collection of vToErase with the write-back of the optimised
 * poses and points.  With them the function is three calls on one stream --
 * gather, orbgpu_local_ba_batch_device unchanged, collect -- with nothing
 * built, uploaded or downloaded between them.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   the local keyframes          src/Optimizer.cpp:540-555
 *   the local MapPoints          src/Optimizer.cpp:557-576
 *   the fixed cameras            src/Optimizer.cpp:578-597
 *   vertices and edges           src/Optimizer.cpp:614-752
 *   vToErase                     src/Optimizer.cpp:813-847
 *   the write-back               src/Optimizer.cpp:849-884
 *
 * What is kept of the reference:
 *   - pKF goes first and is not tested for isBad() (:544);
 *   - a covisible keyframe that is bad is MARKED local (:552) but not listed
 *     (:553-554): it can never become a fixed camera, and being bad it has no
 *     edge either;
 *   - the local points are found by walking the local keyframes in list order
 *     and the slots ascending; NULL slots and bad points are skipped and the
 *     first occurrence of a point decides its position (:560-576);
 *   - the fixed cameras are found by walking the local points in order and
 *     their observations in obs[] order; a keyframe that is not marked local is
 *     marked on first sight and listed only if it is not bad (:590-595);
 *   - one edge per observation whose keyframe is not bad (:688), grouped by
 *     point, within a point in obs[] order;
 *   - an edge takes its keypoint from obs_idx (mit->second, :690), not from the
 *     slot in which the point was found: a point that sits in a keyframe's slot
 *     but lists no observation from that keyframe gets no edge there, and a
 *     local point without observations is a point with no edge;
 *   - edge_pose is the position in the local list, or n_local + the position
 *     in the fixed list (the order the vertices are added in, :618-642);
 *   - obs[2] is -1.0f when mvuRight < 0 (the monocular edge, :693), otherwise
 *     mvuRight: what include/orbslam2_amd/LocalBundleAdjuster.h writes;
 *   - fixed is kf_first (mnId == 0, :624) for a local pose and 1 for a fixed
 *     one (:638);
 *   - mnBALocalForKF / mnBAFixedForKF are compared with pKF's id only, so marks
 *     that are fresh for every job are equivalent;
 *   - vToErase holds the flagged monocular edges in edge order, then the
 *     flagged stereo edges (:818-847).  The pMP->isBad() skip of :823 and :839
 *     cannot fire against a static mirror: the local points are not bad by
 *     construction (:568) and nothing changes the mirror between the gather
 *     and the collection.
 *
 * Order.  obs[] stands for the std::map<KeyFrame*,size_t> order of
 * GetObservations(), as in orbgpu_localmap.h; covis_all is
 * GetVectorCovisibleKeyFrames(), the whole ordered list.
 *
 * The caller's contract: covis_all must not name a keyframe twice and must not
 * name the keyframe it belongs to (the reference's list never does).  If it
 * does, the first occurrence is kept and pKF keeps position 0: a defined
 * result, never a fault.
 *
 * Conventions as in orbgpu.h and orbgpu_localmap.h.  Everything is integers
 * and copied bytes, there is no floating-point arithmetic: a job's outputs are
 * a function of the job and the two mirrors alone, whatever the batch, the
 * job's position or the run.
 */
#ifndef ORBGPU_LOCALBA_MAP_H
#define ORBGPU_LOCALBA_MAP_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu_localba.h"
#include "orbgpu_localmap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- what the gather reads and orbgpu_map_mirror lacks ----------------------
 * A second host struct of device pointers, given beside an orbgpu_map_mirror
 * with the same keyframes, slots and observations.  The caller owns it and
 * keeps it current; the gather does not write it.
 *
 * Keyframes 0..n_kf-1:
 *   covis_all_offset / n_covis_all   GetVectorCovisibleKeyFrames() into
 *                 covis_all[] (n_covis_all_total entries): the whole ordered
 *                 list, not the first 10
 *   kf_first      uint8: mnId == 0
 *   kf_Tcw        float[12]: GetPose(), row-major 3x4
 *   kf_cam        float[5]: fx, fy, cx, cy, mbf
 * Slots, parallel to the first mirror's slots[] (slot s of keyframe k is its
 * keypoint s):
 *   kp_obs        float[3]: mvKeysUn[s].pt.x, .pt.y, mvuRight[s]
 *   kp_inv_sigma2 float: mvInvLevelSigma2[mvKeysUn[s].octave]
 * Observations, parallel to obs[]:
 *   obs_idx       the size_t of GetObservations(): a slot index within that
 *                 keyframe */
typedef struct orbgpu_map_mirror_ba {
    int n_covis_all_total; /* length of covis_all[] */
    int pad;
    const int* covis_all_offset;
    const int* n_covis_all;
    const int* covis_all;
    const uint8_t* kf_first;
    const float* kf_Tcw;
    const float* kf_cam;
    const float* kp_obs;
    const float* kp_inv_sigma2;
    const int* obs_idx;
} orbgpu_map_mirror_ba;

/* The limits of the gather's keys.  A keyframe's first occurrence in
 * covis_all and a point's first (list position, slot) are 32-bit numbers: the
 * slots of one job's local keyframes together must stay below
 * ORBGPU_LOCALBA_MAP_MAX_SLOTS (beyond it the job is CAPACITY with n_points =
 * n_fixed = n_edges = 0, the one case whose counts are not the true ones).  A
 * fixed camera's first sight is a 64-bit (point position, observation
 * position) pair, which no int count exceeds. */
#define ORBGPU_LOCALBA_MAP_MAX_SLOTS 0x7fffffff

enum {
    ORBGPU_LOCALBA_MAP_OK = 0,
    ORBGPU_LOCALBA_MAP_CAPACITY = 2, /* ORBGPU_LOCALMAP_CAPACITY: a list exceeds its stride, see below  */
    ORBGPU_LOCALBA_MAP_BAD_JOB = 3   /* ORBGPU_LOCALMAP_BAD_JOB: an id or offset the job reads lies
                                        outside the mirror (kf, a covis_all entry, a slot, an
                                        observation, an offset + count beyond its array), or the obs_idx
                                        of an edge lies outside its keyframe's slots.  Only the result
                                        (its counts all 0) and the prepared job are written            */
};

typedef struct orbgpu_localba_gather_job {
    int kf; /* pKF's index in the mirror */
    int pad;
} orbgpu_localba_gather_job;

/* CAPACITY: n_local > kf_stride, n_local + n_fixed > pose_stride, n_points >
 * point_stride or n_edges > edge_stride.  Every count is the true one and every
 * array holds its first `stride` entries: local_kfs the first kf_stride local
 * keyframes, the pose arrays the first pose_stride poses (the local ones, then
 * the fixed ones), fixed_kfs the fixed keyframes among those, the point arrays
 * the first point_stride points, the edge arrays the first edge_stride edges
 * (edge_pose and edge_point are the true indices, which may exceed the
 * strides).
 * Under CAPACITY and BAD_JOB the prepared orbgpu_localba_job gets n_poses =
 * n_local = n_points = n_edges = -1 (its offsets are the job's), so
 * orbgpu_local_ba_batch_device reports rounds = -1 for exactly those jobs and
 * reads nothing of theirs, and the collection gives n_erase = 0 for them. */
typedef struct orbgpu_localba_gather_result {
    int status;   /* ORBGPU_LOCALBA_MAP_*                                  */
    int n_local;  /* lLocalKeyFrames.size()                                */
    int n_fixed;  /* lFixedCameras.size()                                  */
    int n_points; /* lLocalMapPoints.size()                                */
    int n_edges;  /* vpEdgesMono.size() + vpEdgesStereo.size()             */
    int n_mono;   /* vpEdgesMono.size()                                    */
    int n_stereo; /* vpEdgesStereo.size()                                  */
    int pad;
} orbgpu_localba_gather_result;

/* Bytes of workspace a gather of n jobs on a mirror of n_kf keyframes and n_pt
 * points needs: a few words per job and mirror keyframe and per job and mirror
 * point.  0 when n * n_kf or n * n_pt does not fit an int. */
size_t orbgpu_local_ba_gather_workspace_bytes(int n, int n_kf, int n_pt);

/* Job k owns fixed ranges of the output arrays, so the host knows every total
 * without a download: poses [k * pose_stride, ..), local pose outputs
 * [k * kf_stride, ..), points [k * point_stride, ..), edges [k * edge_stride,
 * ..).  d_ba_jobs[k] is written with those offsets and the true counts; the
 * input arrays of orbgpu_local_ba_batch_device are written in exactly
 * orbgpu_localba.h's layout (d_Tcw, d_fixed, d_cam: n * pose_stride rows; d_Xw:
 * n * point_stride; d_edge_pose, d_edge_point, d_obs, d_inv_sigma2: n *
 * edge_stride), and the lists a write-back needs:
 *   d_local_kfs    int[n][kf_stride]     lLocalKeyFrames
 *   d_fixed_kfs    int[n][pose_stride]   lFixedCameras
 *   d_local_points int[n][point_stride]  lLocalMapPoints, mirror ids
 *   d_edge_kf, d_edge_slot  int[n][edge_stride]  the observing keyframe of an
 *                  edge and its obs_idx
 * The following orbgpu_local_ba_batch_device is called with total_poses = n *
 * pose_stride, total_local = n * kf_stride, total_points = n * point_stride,
 * total_edges = n * edge_stride and max_local = kf_stride.
 * Entries past the counts are not written and nothing is written outside a
 * job's ranges.  `mirror` and `mirror_ba` are host structs; d_workspace (256-
 * byte aligned) need not be zeroed.  Asynchronous on `stream`: several
 * launches, no host synchronisation, none between workgroups inside a launch,
 * no spinning on memory.
 * ORBGPU_ERR_ARG, before the device is looked at: a negative n, a stride that
 * is not positive, n * stride beyond an int, a NULL pointer with n > 0, a
 * NULL mirror or a mirror array the gather reads that is NULL while its count
 * is positive. */
int orbgpu_local_ba_gather_batch_device(int n, const orbgpu_localba_gather_job* d_jobs,
                                        const orbgpu_map_mirror* mirror, const orbgpu_map_mirror_ba* mirror_ba,
                                        int kf_stride, int pose_stride, int point_stride, int edge_stride,
                                        void* d_workspace, orbgpu_localba_gather_result* d_results,
                                        orbgpu_localba_job* d_ba_jobs, float* d_Tcw, uint8_t* d_fixed, float* d_cam,
                                        float* d_Xw, int* d_edge_pose, int* d_edge_point, float* d_obs,
                                        float* d_inv_sigma2, int* d_local_kfs, int* d_fixed_kfs, int* d_local_points,
                                        int* d_edge_kf, int* d_edge_slot, void* stream);

/* After orbgpu_local_ba_batch_device on the same stream.  Reads the gathered
 * jobs, d_obs, d_edge_point, the lists and LBA's d_erase; writes per job
 * vToErase in the reference's order, d_to_erase int[n][edge_stride][3] =
 * (keyframe, mirror point id, slot), and d_n_erase int[n].  A job whose counts
 * are negative or exceed the strides gets n_erase = 0 and nothing else.
 * Entries past n_erase are not written.
 *
 * d_kf_Tcw / d_pos: the mirror's own kf_Tcw (n_kf x 12) and pos (n_pt x 3), or
 * NULL.  When given, rows 0-2 of every local keyframe's d_Tcw_out row and every
 * local point's d_Xw_out row are scattered to them (SetPose, SetWorldPos,
 * :866-884), which keeps the mirror current without an upload; rows of other
 * keyframes and points keep their bytes.  Two jobs of one batch that share a
 * local keyframe or a local point would make that scatter a race: such a
 * batch must pass NULL for both.  Applying the erasures to the mirror's slots
 * and observations stays with the caller, and so does UpdateNormalAndDepth,
 * for which orbgpu_update_normal_and_depth_batch_device exists.
 * ORBGPU_ERR_ARG as above; d_Tcw_out / d_Xw_out may be NULL when d_kf_Tcw /
 * d_pos is. */
int orbgpu_local_ba_collect_batch_device(int n, const orbgpu_localba_job* d_ba_jobs, int kf_stride, int point_stride,
                                         int edge_stride, const float* d_obs, const int* d_edge_point,
                                         const int* d_local_kfs, const int* d_local_points, const int* d_edge_kf,
                                         const int* d_edge_slot, const uint8_t* d_erase, const float* d_Tcw_out,
                                         const float* d_Xw_out, int* d_to_erase, int* d_n_erase, int n_kf, int n_pt,
                                         float* d_kf_Tcw, float* d_pos, void* stream);

#ifdef __cplusplus
}
#endif
#endif
