/*
 * orbgpu_covis.h -- C ABI of the covisibility graph as a table in HBM, beside
 * the map mirror of orbgpu_localmap.h and orbgpu_localba_map.h, and of the
 * three calls that maintain it: KeyFrame::UpdateConnections for a list of
 * keyframes, the judging loop of LocalMapping::KeyFrameCulling, and the
 * covisibility part of KeyFrame::SetBadFlag for a list of keyframes.  The table
 * holds, per keyframe, the arrays that
 * Tracking::UpdateLocalMap (the best 10), the LBA gather (the whole ordered
 * list) and the keyframe database read, so a caller can point those readers at
 * it and they read the lists where they are kept.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   KeyFrame::AddConnection          src/KeyFrame.cpp:140-154
 *   KeyFrame::UpdateBestCovisibles   src/KeyFrame.cpp:161-184
 *   KeyFrame::UpdateConnections      src/KeyFrame.cpp:369-483
 *   LocalMapping::KeyFrameCulling    src/LocalMapping.cpp:802-880
 *   MapPoint::EraseObservation       src/MapPoint.cpp:141-169
 *   KeyFrame::SetBadFlag             src/KeyFrame.cpp:559-585 (the graph: :572-573, :584-585)
 *   KeyFrame::EraseConnection        src/KeyFrame.cpp:677-691
 *
 * What is kept of the reference:
 *   - EraseConnection(this) runs on every keyframe of the erased keyframe's
 *     mConnectedKeyFrameWeights (:572-573), whether or not that keyframe still
 *     holds the reverse connection (a stale one is simply not found, :682);
 *   - the key is removed from the neighbour's row and, only if it was there,
 *     the neighbour's ordered list is rebuilt from its whole row (:689-690);
 *   - the ordered list is std::sort on (weight, KeyFrame*) ascending, then
 *     reversed (:172-179): descending weight, ties in DESCENDING map order.  A
 *     row is kept in map order, so the position in it stands for the pointer
 *     and the key (weight, position) is unique: the bytes do not depend on the
 *     sort;
 *   - then the keyframe's own mConnectedKeyFrameWeights and
 *     mvpOrderedConnectedKeyFrames are cleared (:584-585).
 * The early returns of SetBadFlag (mnId == 0, mbNotErase, :563-569), the
 * erasure of the keyframe's observations (:575-577) and the spanning tree
 * (:587-660) stay with the caller: it lists only keyframes that are erased.
 *
 * UpdateConnections and KeyFrameCulling are described at their calls below.
 *
 * Order.  As in orbgpu_localmap.h the std::map<KeyFrame*,int> order is the
 * caller's: a conn row is in the order that stands for the std::map's, which is
 * the mirror's kf_by_rank (NULL = ascending index): a row is in ascending rank.
 * The position in a rank-ordered row stands for the pointer, so ties of equal
 * weight go in descending rank in an ordered row.
 *
 * Conventions as in orbgpu.h, orbgpu_localmap.h and orbgpu_localba_map.h.
 * Everything is integers, comparisons and copied bytes: every output byte is a
 * function of the list and the table, whatever the run.
 */
#ifndef ORBGPU_COVIS_H
#define ORBGPU_COVIS_H

#include <stddef.h>
#include <stdint.h>

#include "orbgpu_localba_map.h"
#include "orbgpu_localmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBGPU_COVIS_BEST 10           /* ORBGPU_LOCALMAP_COVIS: the columns of covis10 */
#define ORBGPU_COVIS_MAX_STRIDE 1024   /* the largest conn_stride                       */

/* ---- the graph table --------------------------------------------------------
 * A host struct of device pointers.  The caller owns the arrays; unlike the
 * mirrors they are WRITTEN by the library.  Keyframe k owns entries
 * [k * conn_stride, (k + 1) * conn_stride) of the four row arrays:
 *   n_conn / conn_kf / conn_w   mConnectedKeyFrameWeights, n_conn[k] entries in
 *                 the order that stands for the std::map's (see "Order")
 *   n_ord / ord_kf / ord_w      mvpOrderedConnectedKeyFrames / mvOrderedWeights
 *   covis10       int[n_kf][10]: the first 10 of ord_kf, padded with -1.  It may
 *                 be the first mirror's own covis array
 * The erasure writes no entry past the count a row has when the call begins
 * (the entries between a row's new and old count keep whatever the shifts
 * left there); an ord row that UpdateConnections left shorter than its conn
 * row is rebuilt from the whole conn row and may grow up to that row's count.
 * UpdateConnections writes no entry past max(old count, new count) of a row.
 * A caller points
 * orbgpu_map_mirror_ba.covis_all at ord_kf, covis_all_offset[k] = k * conn_stride
 * and n_covis_all at n_ord (n_covis_all_total = n_kf * conn_stride), and the LBA
 * gather reads the lists in place, as orbgpu_kfdb does with the BoW rows.
 * The caller's contract: a row names no keyframe twice and not its own.  A row
 * whose count lies outside [0, conn_stride] is left alone (as a source it is
 * read up to the nearer bound); a row entry outside [0, n_kf) is never used as
 * an index: a defined result, never a fault. */
typedef struct orbgpu_covis_graph {
    int n_kf;
    int conn_stride; /* 1..ORBGPU_COVIS_MAX_STRIDE */
    int* n_conn;
    int* conn_kf;
    int* conn_w;
    int* n_ord;
    int* ord_kf;
    int* ord_w;
    int* covis10;
} orbgpu_covis_graph;

enum {
    ORBGPU_COVIS_OK = 0,
    ORBGPU_COVIS_EMPTY = 1,    /* UpdateConnections with an empty counter (:411): the table is untouched   */
    ORBGPU_COVIS_CAPACITY = 2, /* ORBGPU_LOCALMAP_CAPACITY: a row or a list exceeds its stride, see below  */
    ORBGPU_COVIS_BAD_JOB = 3   /* ORBGPU_LOCALMAP_BAD_JOB: an index outside the table or the mirror.  Only
                                  the status (the result) is written                                      */
};

/* ---- the covisibility part of SetBadFlag -------------------------------------
 * For the keyframes d_kfs[0..n) in order: EraseConnection(this) on every
 * keyframe of its conn row (:572-573) -- the key is removed from that row and,
 * if it was there, the ordered row and covis10 are rebuilt (:677-691) -- then the
 * keyframe's own rows are cleared (:584-585: n_conn = n_ord = 0, covis10 all
 * -1).  The table after the call equals the keyframes erased one after another
 * in list order (two keyframes that name each other, or one listed twice).
 * d_status[i]: ORBGPU_COVIS_OK, or ORBGPU_COVIS_BAD_JOB for an index outside the
 * table.
 * `graph` is a host struct.  Asynchronous on `stream`: one launch of a single
 * workgroup that walks the list in order, its waves over the entries of the
 * erased keyframe's row; no host synchronisation, no spinning on memory.
 * ORBGPU_ERR_ARG, before the device is looked at: a negative n, a NULL pointer
 * with n > 0, a NULL graph, a negative n_kf, conn_stride outside
 * 1..ORBGPU_COVIS_MAX_STRIDE, n_kf * conn_stride beyond an int, or a NULL graph
 * array with n_kf > 0. */
int orbgpu_covis_erase_keyframes_batch_device(int n, const int* d_kfs, const orbgpu_covis_graph* graph,
                                              int* d_status, void* stream);

/* ---- KeyFrame::UpdateConnections (:369-483) ------------------------------------
 * For the keyframes d_kfs[0..n) in list order; the table after the call equals
 * the function called once per list entry, one after another (job 1 may add a
 * connection to job 2's keyframe, whose rows job 2 then replaces).
 *
 * Counting (:388-408).  Every slot of the keyframe is walked; a slot that holds
 * -1 or a point without ORBGPU_PT_VALID is skipped; every observer of the point
 * other than the keyframe itself gets +1.  A point held in two slots counts
 * twice.  kf_bad is not read, as in the reference.  The counts depend on the
 * mirror alone.
 * Empty counter (:411): ORBGPU_COVIS_EMPTY, the table is untouched.
 * Selection (:417-451), th = 15.  kf_max / w_max is the first strict maximum in
 * rank order.  The ordered set is the counted keyframes with count >= 15 or, if
 * there is none, the one pair (w_max, kf_max).
 * Own rows (:469-471).  The keyframe's conn row becomes ALL counted keyframes in
 * rank order.  Its ord row becomes ONLY the ordered set, in descending weight,
 * ties in descending rank, and covis10 the first 10 of that: this ord row is
 * not UpdateBestCovisibles of the conn row.
 * AddConnection(this, w) (:140-154) runs on every member of the ordered set: an
 * absent key is inserted at its rank position in that neighbour's conn row, a
 * present one has its weight overwritten; unless the weight was already w, the
 * neighbour's ord row and covis10 are then rebuilt from its WHOLE conn row.
 * front is the new ord_kf[0]: mbFirstConnection, the parent and the children
 * (:474-481) stay the caller's, as the spanning tree does for SetBadFlag.
 *
 * ORBGPU_COVIS_CAPACITY: more than conn_stride keyframes are counted, or a
 * neighbour that needs an insertion already holds conn_stride entries (or a
 * count outside [0, conn_stride]) in its state after the earlier jobs.  It is
 * decided before the job's first write: the job changes nothing in the table.
 * n_counted, n_ordered, kf_max and w_max are the true ones, front is -1.
 * ORBGPU_COVIS_BAD_JOB: a keyframe index, slot range, point id (other than -1),
 * observation range or observer index outside the mirror or the table, or a
 * kf_by_rank entry outside it (then for every job).  The job writes its result
 * only: n_counted = n_ordered = w_max = 0, kf_max = front = -1, as for EMPTY.
 * Entries past max(old count, new count) of a row are not written. */
typedef struct orbgpu_covis_update_result {
    int status;    /* ORBGPU_COVIS_*                                    */
    int n_counted; /* KFcounter.size(): the new n_conn of the keyframe  */
    int n_ordered; /* vPairs.size(): the new n_ord of the keyframe      */
    int kf_max;    /* pKFmax                                            */
    int w_max;     /* nmax                                              */
    int front;     /* mvpOrderedConnectedKeyFrames.front(), -1 for none */
    int pad[2];
} orbgpu_covis_update_result;

#define ORBGPU_COVIS_TH 15 /* :419 */

/* Bytes of workspace for n jobs on n_kf keyframes: the inverse of kf_by_rank and
 * one counter per job and keyframe.  0 when that does not fit an int, or for a
 * negative argument. */
size_t orbgpu_covis_update_workspace_bytes(int n, int n_kf);

/* `mirror` and `graph` are host structs; of the mirror n_kf, n_pt, n_slots_total,
 * n_obs_total, slot_offset, n_slots, slots, pt_flags, obs_offset, n_obs, obs and
 * kf_by_rank are read.  d_workspace (4-byte aligned, workspace_bytes long) need
 * not be zeroed.  Asynchronous on `stream`: the counts of all jobs in parallel
 * with integer atomics, then one launch of a single workgroup that applies the
 * jobs in list order, a wave per neighbour; no host synchronisation, no
 * spinning on memory.
 * ORBGPU_ERR_ARG, before the device is looked at: what the erasure refuses, a
 * NULL mirror or result pointer with n > 0, mirror->n_kf != graph->n_kf, a
 * negative count of the mirror, a mirror array that is read and is NULL while
 * its count is positive, a NULL workspace or workspace_bytes below
 * orbgpu_covis_update_workspace_bytes(n, n_kf) (which is 0 when it does not fit). */
int orbgpu_covis_update_connections_batch_device(int n, const int* d_kfs, const orbgpu_map_mirror* mirror,
                                                 const orbgpu_covis_graph* graph, void* d_workspace,
                                                 size_t workspace_bytes, orbgpu_covis_update_result* d_results,
                                                 void* stream);

/* ---- the judging loop of LocalMapping::KeyFrameCulling (:802-880) ---------------
 * What the judge reads beside orbgpu_map_mirror and orbgpu_map_mirror_ba (of
 * which kf_first, kp_obs and obs_idx are read): a third host struct of device
 * pointers, the caller's, never written.
 *   kp_octave     uint8, parallel to slots[]: mvKeysUn[s].octave
 *   kp_depth      float, parallel to slots[]: mvDepth[s]
 *   kf_th_depth   float per keyframe: mThDepth
 *   kf_not_erase  uint8 per keyframe: mbNotErase */
typedef struct orbgpu_map_mirror_cull {
    const uint8_t* kp_octave;
    const float* kp_depth;
    const float* kf_th_depth;
    const uint8_t* kf_not_erase;
} orbgpu_map_mirror_cull;

typedef struct orbgpu_covis_cull_job {
    int kf;   /* mpCurrentKeyFrame's index */
    int mono; /* mbMonocular               */
} orbgpu_covis_cull_job;

enum {
    ORBGPU_COVIS_CULL_KEPT = 0,          /* judged and not redundant                                */
    ORBGPU_COVIS_CULL_CULLED = 1,        /* SetBadFlag() erases it                                  */
    ORBGPU_COVIS_CULL_TO_BE_ERASED = 2,  /* redundant, but mbNotErase: mbToBeErased is set (:565-569) */
    ORBGPU_COVIS_CULL_SKIPPED_FIRST = 3  /* mnId == 0 (:816)                                        */
};

typedef struct orbgpu_covis_cull_verdict {
    int kf;
    int n_mps;       /* nMPs                   */
    int n_redundant; /* nRedundantObservations */
    int verdict;     /* ORBGPU_COVIS_CULL_*    */
} orbgpu_covis_cull_verdict;

typedef struct orbgpu_covis_cull_result {
    int status;         /* ORBGPU_COVIS_OK, _CAPACITY or _BAD_JOB                    */
    int n_list;         /* vpLocalKeyFrames.size(): n_ord of the job's keyframe      */
    int n_culled;       /* verdicts CULLED                                           */
    int n_to_be_erased; /* verdicts TO_BE_ERASED                                     */
    int pad[4];
} orbgpu_covis_cull_result;

/* n independent jobs.  The list of a job is its keyframe's ord row as it stands
 * when the call begins (GetVectorCovisibleKeyFrames, :810); nothing more of the
 * graph is read, since an erased connection never changes a later verdict, and
 * nothing is written to the graph or the mirrors.  Per list entry, in order:
 *   - kf_first set: SKIPPED_FIRST (:816);
 *   - otherwise every slot of the entry's keyframe is walked.  A -1 slot, a point
 *     without ORBGPU_PT_VALID and a point the job's earlier verdicts made bad
 *     (below) are skipped; when the job is not monocular a slot is skipped when
 *     depth > th_depth || depth < 0, as floats (:837); then nMPs++.  A point's
 *     nObs is derived here: over its current observations, 2 where
 *     kp_obs[slot][2] >= 0 and 1 otherwise (MapPoint::AddObservation).  If nObs > 3
 *     the point is redundant when at least 3 of its current observers other than
 *     the judged keyframe have octave_i <= octave + 1 (:843-870);
 *   - the entry is redundant when (double)nRedundant > 0.9 * (double)nMPs (:877).
 *     With kf_not_erase set it gets TO_BE_ERASED and changes nothing; otherwise
 *     CULLED, and for the job's later verdicts it is no longer an observer of
 *     any point: its 1 or 2 leaves the point's nObs, and a point that has lost
 *     at least one observer and whose nObs is then <= 2 is bad
 *     (MapPoint::EraseObservation :162), which is NULL in every later slot.
 * The caller's contract: obs[] / obs_idx[] and slots[] agree with each other (a
 * keyframe is an observer of exactly the points in its slots) and the list
 * names no keyframe twice.
 * Outputs per job k: d_results[k]; d_verdicts[k * list_stride + e] for e <
 * n_list, status OK only; d_culled[k * list_stride + e] for EVERY e <
 * list_stride: the keyframe where the verdict is CULLED, else -1 (all -1 under
 * CAPACITY and BAD_JOB).  d_culled goes unchanged as d_kfs, with n = (jobs *)
 * list_stride, to orbgpu_covis_erase_keyframes_batch_device on the same stream,
 * where a -1 is a BAD_JOB that writes its status only: the graph side of
 * KeyFrameCulling is two calls with no host read between them.  Replaying the
 * observations, kf_bad and the spanning tree on the mirror stays the caller's.
 * ORBGPU_COVIS_CAPACITY: n_list > list_stride (n_list is the true one).
 * ORBGPU_COVIS_BAD_JOB: kf, a list entry or n_ord outside the table, a slot
 * range, point id (other than -1), observation range, observer or obs_idx
 * outside the mirror.  n_list = n_culled = n_to_be_erased = 0.
 * Asynchronous on `stream`: one launch, a workgroup per job that walks its list
 * in order, its waves over the slots of the judged keyframe; the culled set (at
 * most conn_stride keyframes) is kept in LDS.  No spinning on memory, integer
 * atomics only.
 * ORBGPU_ERR_ARG, before the device is looked at: what the erasure refuses, a
 * NULL pointer with n > 0, list_stride < 1, n * list_stride beyond an int,
 * mirror->n_kf != graph->n_kf, a negative count of the mirror, or a mirror array
 * that is read and is NULL while its count is positive. */
int orbgpu_covis_keyframe_culling_batch_device(int n, const orbgpu_covis_cull_job* d_jobs,
                                               const orbgpu_map_mirror* mirror,
                                               const orbgpu_map_mirror_ba* mirror_ba,
                                               const orbgpu_map_mirror_cull* mirror_cull,
                                               const orbgpu_covis_graph* graph, int list_stride,
                                               orbgpu_covis_cull_result* d_results,
                                               orbgpu_covis_cull_verdict* d_verdicts, int* d_culled, void* stream);

#ifdef __cplusplus
}
#endif
#endif
