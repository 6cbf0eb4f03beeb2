/*
 * orbgpu_covis.h -- C ABI of the covisibility graph as a table in HBM, beside
 * the map mirror of orbgpu_localmap.h and orbgpu_localba_map.h, and of the one
 * call that maintains it so far: the covisibility part of KeyFrame::SetBadFlag
 * for a list of keyframes.  The table holds, per keyframe, the arrays that
 * Tracking::UpdateLocalMap (the best 10), the LBA gather (the whole ordered
 * list) and the keyframe database read, so a caller can point those readers at
 * it and they read the lists where they are kept.
 *
 * Reference (paths relative to ORB-SLAM2/):
 *   KeyFrame::UpdateBestCovisibles   src/KeyFrame.cpp:161-184
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
 * Not here yet: KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling
 * on the device.  The caller fills the rows as before, whenever
 * UpdateBestCovisibles runs for a keyframe.
 *
 * Order.  As in orbgpu_localmap.h the std::map<KeyFrame*,int> order is the
 * caller's: a conn row is given in the order that stands for the std::map's.
 *
 * Conventions as in orbgpu.h, orbgpu_localmap.h and orbgpu_localba_map.h.
 * Everything is integers, comparisons and copied bytes: every output byte is a
 * function of the list and the table, whatever the run.
 */
#ifndef ORBGPU_COVIS_H
#define ORBGPU_COVIS_H

#include <stddef.h>
#include <stdint.h>

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
 * Entries past the count a row has when a call begins are not written by it
 * (the entries between a row's new and old count keep whatever the shifts
 * left there).  A caller points
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
    ORBGPU_COVIS_BAD_JOB = 3 /* ORBGPU_LOCALMAP_BAD_JOB: an index outside the table.  Only the status is written */
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

#ifdef __cplusplus
}
#endif
#endif
