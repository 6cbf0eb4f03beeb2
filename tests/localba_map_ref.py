"""Restatement of the two host stretches of Optimizer::LocalBundleAdjustment
(src/Optimizer.cpp:540-752 and :813-847) against the map mirror, for
include/orbgpu_localba_map.h and csrc/localba_map.hip: the reference's loops as
the reference writes them -- Python lists and marks, one job at a time.

A map is two dicts.  `mirror` is tests/localmap_ref.py's (kf_bad, slots,
pt_flags, obs, pos ..); `ba` holds what orbgpu_map_mirror_ba adds: covis_all
(per keyframe a list), kf_first, kf_Tcw (n_kf, 12), kf_cam (n_kf, 5), kp_obs /
kp_inv_sigma2 (per keyframe arrays parallel to its slots), obs_idx (per point a
list parallel to its observations).

``gather`` returns every output array, count and status, with the CAPACITY
truncation and BAD_JOB of the header; ``collect`` returns vToErase.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

OK, CAPACITY, BAD_JOB = 0, 2, 3  # ORBGPU_LOCALBA_MAP_*
VALID = 1                        # ORBGPU_PT_VALID
F32 = np.float32


def _bad_job():
    z = lambda dt, *shape: np.zeros((0,) + shape, dt)
    return SimpleNamespace(status=BAD_JOB, n_local=0, n_fixed=0, n_points=0, n_edges=0, n_mono=0, n_stereo=0,
                           local_kfs=[], fixed_kfs=[], local_points=[], Tcw=z(F32, 12), fixed=z(np.uint8),
                           cam=z(F32, 5), Xw=z(F32, 3), edge_pose=z(np.int32), edge_point=z(np.int32), obs=z(F32, 3),
                           inv_sigma2=z(F32), edge_kf=z(np.int32), edge_slot=z(np.int32), counts=(-1, -1, -1, -1),
                           full=None)


def gather(mirror, ba, kf, kf_stride, pose_stride, point_stride, edge_stride):
    """One job.  The namespace's arrays are what the device writes (under CAPACITY the first `stride`
    entries); `full` holds the untruncated lists and arrays, `counts` the prepared orbgpu_localba_job's
    (n_poses, n_local, n_points, n_edges)."""
    bad, slots, obs_of = mirror["kf_bad"], mirror["slots"], mirror["obs"]
    n_kf, n_pt = len(bad), len(mirror["pt_flags"])
    pKF = int(kf)
    if not 0 <= pKF < n_kf:
        return _bad_job()
    # Local KeyFrames (:540-555).  mnBALocalForKF: a keyframe marked twice (covis_all naming one twice, or
    # pKF) keeps its first mark -- the header's defined result for a list the reference never produces
    local_mark = {pKF}
    lLocalKeyFrames = [pKF]
    for pKFi in (int(v) for v in ba["covis_all"][pKF]):
        if not 0 <= pKFi < n_kf:
            return _bad_job()
        if pKFi in local_mark:
            continue
        local_mark.add(pKFi)  # marked whether bad or not (:552)
        if not bad[pKFi]:
            lLocalKeyFrames.append(pKFi)
    # Local MapPoints seen in Local KeyFrames (:557-576)
    point_mark = set()
    lLocalMapPoints = []
    broken = False
    for k in lLocalKeyFrames:
        for pMP in (int(v) for v in slots[k]):
            if pMP == -1:
                continue
            if not 0 <= pMP < n_pt:
                broken = True  # the device checks every slot of every local keyframe
                continue
            if mirror["pt_flags"][pMP] & VALID and pMP not in point_mark:
                lLocalMapPoints.append(pMP)
                point_mark.add(pMP)
    if broken:
        return _bad_job()
    # Fixed Keyframes (:578-597)
    fixed_mark = set()
    lFixedCameras = []
    for pMP in lLocalMapPoints:
        for pKFi in (int(v) for v in obs_of[pMP]):
            if not 0 <= pKFi < n_kf:
                return _bad_job()
            if pKFi not in local_mark and pKFi not in fixed_mark:
                fixed_mark.add(pKFi)
                if not bad[pKFi]:
                    lFixedCameras.append(pKFi)
    # vertices (:614-642): the local poses, then the fixed ones
    poses = lLocalKeyFrames + lFixedCameras
    vertex = {k: i for i, k in enumerate(poses)}
    Tcw = np.asarray(ba["kf_Tcw"], F32).reshape(-1, 12)[poses].reshape(-1, 12)
    cam = np.asarray(ba["kf_cam"], F32).reshape(-1, 5)[poses].reshape(-1, 5)
    fixed = np.array([1 if ba["kf_first"][k] else 0 for k in lLocalKeyFrames] + [1] * len(lFixedCameras), np.uint8)
    Xw = np.asarray(mirror["pos"], F32).reshape(-1, 3)[lLocalMapPoints].reshape(-1, 3)
    # edges (:669-752)
    e_pose, e_point, e_obs, e_sig, e_kf, e_slot = [], [], [], [], [], []
    n_mono = 0
    for m, pMP in enumerate(lLocalMapPoints):
        for pKFi, idx in zip((int(v) for v in obs_of[pMP]), (int(v) for v in ba["obs_idx"][pMP])):
            if bad[pKFi]:
                continue  # :688
            if not 0 <= idx < len(slots[pKFi]):
                return _bad_job()
            x, y, ur = (F32(v) for v in np.asarray(ba["kp_obs"][pKFi], F32).reshape(-1, 3)[idx])
            mono = bool(ur < 0)  # :693
            n_mono += mono
            e_pose.append(vertex[pKFi])
            e_point.append(m)
            e_obs.append((x, y, F32(-1.0) if mono else ur))
            e_sig.append(np.asarray(ba["kp_inv_sigma2"][pKFi], F32).reshape(-1)[idx])
            e_kf.append(pKFi)
            e_slot.append(idx)
    n_local, n_fixed, n_points, n_edges = len(lLocalKeyFrames), len(lFixedCameras), len(lLocalMapPoints), len(e_pose)
    full = SimpleNamespace(local_kfs=lLocalKeyFrames, fixed_kfs=lFixedCameras, local_points=lLocalMapPoints, Tcw=Tcw,
                           fixed=fixed, cam=cam, Xw=Xw, edge_pose=np.array(e_pose, np.int32),
                           edge_point=np.array(e_point, np.int32), obs=np.array(e_obs, F32).reshape(-1, 3),
                           inv_sigma2=np.array(e_sig, F32), edge_kf=np.array(e_kf, np.int32),
                           edge_slot=np.array(e_slot, np.int32))
    over = n_local > kf_stride or n_local + n_fixed > pose_stride or n_points > point_stride or n_edges > edge_stride
    P, M, E = pose_stride, point_stride, edge_stride
    return SimpleNamespace(
        status=CAPACITY if over else OK, n_local=n_local, n_fixed=n_fixed, n_points=n_points, n_edges=n_edges,
        n_mono=n_mono, n_stereo=n_edges - n_mono, local_kfs=lLocalKeyFrames[:kf_stride],
        fixed_kfs=lFixedCameras[:max(P - n_local, 0)], local_points=lLocalMapPoints[:M], Tcw=Tcw[:P], fixed=fixed[:P],
        cam=cam[:P], Xw=Xw[:M], edge_pose=full.edge_pose[:E], edge_point=full.edge_point[:E], obs=full.obs[:E],
        inv_sigma2=full.inv_sigma2[:E], edge_kf=full.edge_kf[:E], edge_slot=full.edge_slot[:E],
        counts=(-1, -1, -1, -1) if over else (n_local + n_fixed, n_local, n_points, n_edges), full=full)


def collect(g, erase):
    """vToErase (:813-847) of a gathered job and LBA's erase flags: (keyframe, mirror point id, slot) of the
    flagged monocular edges in edge order, then of the flagged stereo edges.  A job that is not OK erases
    nothing.  pMP->isBad() (:823, :839) cannot fire: the local points are not bad (:568)."""
    if g.status != OK:
        return []
    erase = np.asarray(erase).astype(bool)
    mono = g.obs[:, 2] < 0
    out = []
    for cls in (True, False):
        for e in range(g.n_edges):
            if erase[e] and bool(mono[e]) == cls:
                out.append((int(g.edge_kf[e]), int(g.local_points[g.edge_point[e]]), int(g.edge_slot[e])))
    return out


def problem(g):
    """a gathered job as a localba.make_batch problem"""
    return dict(Tcw=g.Tcw, fixed=g.fixed, cam=g.cam, Xw=g.Xw, pose_idx=g.edge_pose, point_idx=g.edge_point, obs=g.obs,
                inv_sigma2=g.inv_sigma2, n_local=g.n_local)
