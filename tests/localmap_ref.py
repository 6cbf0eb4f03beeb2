"""Tracking::UpdateLocalMap restated literally (src/Tracking.cpp:1571-1745) for
include/orbgpu_localmap.h: UpdateLocalKeyFrames' vote, K1, the K2 walk and
UpdateLocalPoints as the reference writes them, with Python dicts and lists
iterated the way the reference iterates its std::map / std::set / std::vector,
followed by the table, frame_mp and counts that orbgpu_update_local_map_batch_device
hands to call 2.

Inputs (tests/localmap_scene.py builds them):

  mirror   dict: kf_bad (n_kf,) u8; slots: per keyframe an int array (point id or
           -1); covis (n_kf, 10) int, -1 padded; children: per keyframe a list;
           parent (n_kf,) int; kf_by_rank: None or a permutation; pt_flags (n_pt,)
           int32 of VALID / HAS_OBS; obs: per point a list of keyframes; pos,
           normal (n_pt, 3) f32; desc (n_pt, 32) u8; min_dist, max_dist (n_pt,) f32
  job      dict: n_kp; rows (2, >= n_kp) int32, call 1's; src_pt_id (src_n,) int32;
           src_pos (src_n, 3) f32; src_desc (src_n, 32) u8; prev_kfs: a list

The order of the std::map<KeyFrame*,int> is kf_by_rank's (None: ascending index)
and the order of a std::set<KeyFrame*> of children is the list's: the heap-address
order of the reference is the caller's to state.

An id outside the mirror ends the job as BAD_JOB exactly where the device meets
it: the ids of the rows, of the held good points' observations, of kf_by_rank,
of the previous list on the empty-vote path, of every keyframe the K2 walk
visits (all ten covisibles, all children, the parent) and of every local
keyframe's slots.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

OK, KEPT, CAPACITY, BAD_JOB = range(4)
VALID, HAS_OBS, LAST_SEEN = 1, 2, 8
MAX_KPS = 4096


class BadJob(Exception):
    pass


def _check(ok):
    if not ok:
        raise BadJob


def update_local_keyframes(M, mp, prev_kfs):
    """:1622-1745.  mp: the frame's mvpMapPoints as mirror ids (None, or -1 for a temporal point), nulled in
    place.  Returns (kept, n_k1, mvpLocalKeyFrames, pKFmax or -1, nulled keypoints)."""
    n_kf, bad = len(M["kf_bad"]), M["kf_bad"]
    rank = list(range(n_kf)) if M.get("kf_by_rank") is None else [int(k) for k in M["kf_by_rank"]]
    keyframe_counter, nulled = {}, []
    for i in range(len(mp)):
        if mp[i] is None or mp[i] < 0:  # NULL, or a temporal point: never bad, no observations
            continue
        if M["pt_flags"][mp[i]] & VALID:
            for kf in M["obs"][mp[i]]:
                _check(0 <= kf < n_kf)
                keyframe_counter[kf] = keyframe_counter.get(kf, 0) + 1
        else:
            mp[i] = None  # :1641
            nulled.append(i)
    for kf in rank:
        _check(0 <= kf < n_kf)
    if not keyframe_counter:  # :1646
        for kf in prev_kfs:
            _check(0 <= kf < n_kf)
        return True, 0, [int(k) for k in prev_kfs], -1, nulled
    order = {kf: r for r, kf in enumerate(rank)}
    vmax, kf_max = 0, -1
    local, mark = [], set()
    for kf in sorted(keyframe_counter, key=order.__getitem__):  # the std::map's iteration
        if bad[kf]:
            continue
        if keyframe_counter[kf] > vmax:
            vmax, kf_max = keyframe_counter[kf], kf
        local.append(kf)
        mark.add(kf)
    n_k1 = len(local)
    for it in range(n_k1):  # itEndKF is taken before anything is appended
        if len(local) > 80:
            break
        kf = local[it]
        neighs = [int(c) for c in M["covis"][kf][:10]]
        childs, parent = [int(c) for c in M["children"][kf]], int(M["parent"][kf])
        for c in neighs:
            _check(-1 <= c < n_kf)
        for c in childs:
            _check(0 <= c < n_kf)
        _check(-1 <= parent < n_kf)
        for c in neighs:
            if c >= 0 and not bad[c] and c not in mark:
                local.append(c)
                mark.add(c)
                break
        for c in childs:
            if not bad[c] and c not in mark:
                local.append(c)
                mark.add(c)
                break
        if parent >= 0 and parent not in mark:  # not tested for isBad(); the break leaves the outer loop
            local.append(parent)
            mark.add(parent)
            break
    return False, n_k1, local, kf_max, nulled


def update_local_points(M, local_kfs):
    """:1588-1615"""
    n_pt = len(M["pt_flags"])
    points, mark = [], set()
    for kf in local_kfs:
        for p in M["slots"][kf]:
            p = int(p)
            if p == -1:
                continue
            _check(0 <= p < n_pt)
            if p in mark:
                continue
            if M["pt_flags"][p] & VALID:
                points.append(p)
                mark.add(p)
    return points


def update_local_map(M, J, stride, point_stride, kf_stride):
    """One job.  Returns a namespace: status, n_k1, n_local_kfs, ref_kf, n_nulled, n_local, n_extra, local_kfs,
    local_points (whole lists), frame_mp (n_kp,), table {flags, pos, normal, desc, min_dist, max_dist} of all
    n_local + n_extra entries -- under CAPACITY the device writes the first point_stride / kf_stride of them --
    and points_n, n_local_job: what the prepared job gets."""
    n_kp, n_pt = int(J["n_kp"]), len(M["pt_flags"])
    out = SimpleNamespace(status=OK, n_k1=0, n_local_kfs=0, ref_kf=-1, n_nulled=0, n_local=0, n_extra=0, local_kfs=[],
                          local_points=[], frame_mp=np.full(max(n_kp, 0), -1, np.int32), table=None, points_n=0,
                          n_local_job=0)
    if n_kp > min(stride, MAX_KPS):
        out.status, out.points_n = CAPACITY, point_stride + 1
        return out
    src = np.asarray(J["src_pt_id"], np.int32)
    rows = np.asarray(J["rows"], np.int32)
    try:
        mp, before = [], set()
        for j in range(n_kp):
            t0, t1 = int(rows[0][j]), int(rows[1][j])
            if t0 >= 0:
                _check(t0 < len(src) and -1 <= src[t0] < n_pt)
                before.add(int(src[t0]))
            if t1 >= 0:
                _check(t1 < len(src) and -1 <= src[t1] < n_pt)
                _check(src[t1] >= 0 or (J.get("src_pos") is not None and J.get("src_desc") is not None))
            mp.append(int(src[t1]) if t1 >= 0 else None)
        kept, out.n_k1, kfs, out.ref_kf, nulled = update_local_keyframes(M, mp, J.get("prev_kfs", []))
        if len(kfs) > kf_stride:
            out.status, out.n_local_kfs, out.local_kfs, out.n_nulled = CAPACITY, len(kfs), kfs, len(nulled)
            out.points_n = point_stride + 1
            return out
        points = update_local_points(M, kfs)
    except BadJob:
        return SimpleNamespace(status=BAD_JOB, n_k1=0, n_local_kfs=0, ref_kf=-1, n_nulled=0, n_local=0, n_extra=0,
                               local_kfs=[], local_points=[], frame_mp=None, table=None, points_n=None, n_local_job=None)
    out.n_local_kfs, out.local_kfs, out.n_nulled = len(kfs), kfs, len(nulled)
    out.n_local, out.local_points = len(points), points
    # the table: the local points, then what the frame holds beside them, in keypoint order and once each
    index = {p: i for i, p in enumerate(points)}
    after = {p for p in mp if p is not None and p >= 0}
    entries = [("map", p, VALID | (int(M["pt_flags"][p]) & HAS_OBS) | (LAST_SEEN if p in before and p not in after else 0))
               for p in points]
    extra = {}
    for j in range(n_kp):
        if mp[j] is None:
            continue
        key = ("map", mp[j]) if mp[j] >= 0 else ("vo", int(rows[1][j]))
        if key[0] == "map" and mp[j] in index:
            out.frame_mp[j] = index[mp[j]]
            continue
        if key not in extra:
            extra[key] = len(entries)
            entries.append((key[0], key[1], VALID | (int(M["pt_flags"][mp[j]]) & HAS_OBS) if mp[j] >= 0 else VALID))
        out.frame_mp[j] = extra[key]
    out.n_extra = len(extra)
    n = len(entries)
    T = {"flags": np.zeros(n, np.int32), "pos": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32),
         "desc": np.zeros((n, 32), np.uint8), "min_dist": np.zeros(n, np.float32), "max_dist": np.zeros(n, np.float32)}
    for i, (kind, p, fl) in enumerate(entries):
        T["flags"][i] = fl
        if kind == "map":
            for name in ("pos", "normal", "desc", "min_dist", "max_dist"):
                T[name][i] = M[name][p]
        else:  # call 1's entry; the normal and the distances of a held point are never read: zeros
            T["pos"][i], T["desc"][i] = J["src_pos"][p], J["src_desc"][p]
    out.table, out.points_n, out.n_local_job = T, n, len(points)
    out.status = CAPACITY if n > point_stride else (KEPT if kept else OK)
    return out
