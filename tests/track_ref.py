"""CPU restatement of Tracking's per-frame chain (src/Tracking.cpp:977-1025,
:1033-1114, :1126-1198, :1210-1264, :1496-1562): the reference for
csrc/track.hip.  It composes the oracle's pieces -- proj_ref's LAST_FRAME and
LOCAL SearchByProjection and isInFrustum, poseopt_ref's PoseOptimization -- on
tests/track_scene.py scenes, as reloc_ref.py composes its own, and adds the
literal UpdateLastFrame loop with Frame::UnprojectStereo (src/Frame.cpp:780-796).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import poseopt_ref
import proj_ref
import track_scene as ts

F32, F64 = np.float32, np.float64
OK, FEW_MATCHES, LOST, CAPACITY, BAD_JOB = range(5)
VALID, HAS_OBS, IN_VIEW, LAST_SEEN = 1, 2, 4, 8
PT_SEEN, PT_IN_VIEW = 1, 2


def _pose_optimization(f, stereo, mp, pos, Tcw):
    """Optimizer::PoseOptimization(&mCurrentFrame): the gather over the keypoints with a MapPoint, ascending"""
    k = f["kps"]
    gidx = np.nonzero(mp >= 0)[0]
    Xw = pos[mp[gidx]].astype(F32).reshape(-1, 3)
    ur = f["u_right"][gidx] if f["u_right"] is not None else np.full(len(gidx), -1.0, F32)
    obs = np.stack([k["x"][gidx], k["y"][gidx], ur], 1).astype(F32).reshape(-1, 3)
    w = ts.INV_SIGMA2[k["octave"][gidx]]
    o = poseopt_ref.pose_optimization(np.asarray(Tcw, F32)[:3], Xw, obs, w, ts.K, ts.BF if stereo else 0.0)
    o.gidx = gidx
    o.margin = poseopt_ref.threshold_margin(o, obs)
    return o


def track_initial(batch, j):
    """TrackWithMotionModel (:1139-1197) / TrackReferenceKeyFrame (:992-1024) for job j of a
    track_scene.initial_batch.  Returns a namespace: status, searches, nsearch [2] (-1: not run), nmatches,
    nmatches_map, vo, opt (None: no optimisation), Tcw, rows [2] (mvpMapPoints before / after the cull, all
    -1 without an optimisation), calls (per search: th, the occupancy it saw, its raw row), counts (every
    (value, threshold) the control flow compared)."""
    J = batch["jobs"][j]
    f, stereo, tab = batch["frames"][J["frame"]], batch["stereo"], J["table"]
    n = len(f["kps"])
    out = SimpleNamespace(status=OK, searches=0, nsearch=[-1, -1], nmatches=0, nmatches_map=0, vo=0, opt=None,
                          Tcw=np.asarray(J["Tcw_init"], F32), rows=[np.full(n, -1, np.int32)] * 2, calls=[], counts=[])
    mp = np.full(n, -1, np.int32)  # fill(mvpMapPoints, NULL) (:1141)
    if J["mode"] == 0:
        pts = {"flags": tab["flags"], "pos": tab["pos"], "desc": tab["desc"], "octave": tab["octave"],
               "angle": tab["angle"]}
        th = J["th"]
        for attempt in range(2):
            occ = np.where(mp >= 0, 1, 0).astype(np.uint8)  # NULL everywhere: both calls start from a filled row
            tgt = ts.frame_target(f, stereo, J["Tcw_init"], occ)
            nm, m = proj_ref.search_by_projection(proj_ref.LAST_FRAME, tgt, pts, th, nnratio=0.9, check_ori=True,
                                                  mono=bool(J["mono"]), last_Tcw=J["last_Tcw"])
            out.calls.append({"th": th, "occupied": occ.copy(), "row": m.copy()})
            out.nsearch[attempt] = nm
            out.searches += 1
            out.counts.append((nm, 20))
            if nm >= 20:
                break
            mp[:] = -1  # :1158
            th = 2 * th
        few = nm < 20
        if not few:
            mp = np.where(m >= 0, m, -1).astype(np.int32)  # a -2 was the call's own culled assignment
    else:
        nm = int(J["bow_nmatches"])
        out.counts.append((nm, 15))
        few = nm < 15
        if not few:
            mp = np.asarray(J["bow_row"], np.int32).copy()
    out.nmatches = nm
    if few:
        out.status = FEW_MATCHES
        return out
    before = mp.copy()
    o = _pose_optimization(f, stereo, mp, tab["pos"], J["Tcw_init"])
    outlier = np.zeros(n, bool)
    outlier[o.gidx] = o.outlier
    nmap = 0
    for i in range(n):  # :1172-1189
        if mp[i] >= 0:
            if outlier[i]:
                mp[i] = -1
                nm -= 1
            elif tab["flags"][mp[i]] & HAS_OBS:
                nmap += 1
    out.opt, out.Tcw, out.rows = o, o.Tcw, [before, mp.copy()]
    out.nmatches, out.nmatches_map = nm, nmap
    if J["mode"] == 0 and J["only_tracking"]:
        out.vo = int(nmap < 10)
        ok = nm > 20
        out.counts += [(nm, 20), (nmap, 10)]
    else:
        ok = nmap >= 10
        out.counts.append((nmap, 10))
    out.status = OK if ok else LOST
    return out


def track_local(batch, j, Tcw=None):
    """SearchLocalPoints (:1501-1561) + TrackLocalMap (:1225-1263) for job j of a track_scene.local_batch from
    the pose Tcw (default the job's).  Returns a namespace: status, n_to_match, nsearch (-1: not run),
    n_inliers, opt, Tcw, rows [3] (mvpMapPoints after the search, at the end; mvbOutlier), point_flags,
    in_frustum (what isInFrustum says of every local point, seen or not), counts."""
    J = batch["jobs"][j]
    f, stereo, tab = batch["frames"][J["frame"]], batch["stereo"], J["table"]
    Tcw = np.asarray(J["Tcw"] if Tcw is None else Tcw, F32).reshape(4, 4)
    n, nl = len(f["kps"]), J["n_local"]
    flags = np.asarray(tab["flags"], np.int32)
    mp = np.asarray(J["frame_mp"], np.int32).copy()
    pf = np.zeros(len(flags), np.uint8)
    for i in range(n):  # :1501-1520
        if mp[i] >= 0:
            if not flags[mp[i]] & VALID:
                mp[i] = -1
            else:
                pf[mp[i]] = PT_SEEN
    loc = {k: v[:nl] for k, v in tab.items()}
    tgt = ts.frame_target(f, stereo, Tcw, None)
    fl_all, track, level = proj_ref.is_in_frustum(tgt, dict(loc, flags=flags[:nl] & (VALID | HAS_OBS)), 0.5)
    # :1526-1545; mnLastFrameSeen == mnId (:1531) for the held points and for those call 1 culled (:1016, :1183)
    to_match = (flags[:nl] & VALID).astype(bool) & ((flags[:nl] & LAST_SEEN) == 0) & (pf[:nl] == 0) & \
        ((fl_all & IN_VIEW) != 0)
    pf[:nl][to_match] = PT_IN_VIEW
    out = SimpleNamespace(n_to_match=int(to_match.sum()), nsearch=-1, in_frustum=(fl_all & IN_VIEW) != 0, counts=[])
    if out.n_to_match > 0:
        occ = np.array([0 if p < 0 else (2 if flags[p] & HAS_OBS else 1) for p in mp], np.uint8)
        pts = dict(loc, flags=(flags[:nl] & (VALID | HAS_OBS)) | np.where(to_match, IN_VIEW, 0), track=track,
                   track_level=level)
        out.nsearch, m = proj_ref.search_by_projection(proj_ref.LOCAL, dict(tgt, occupied=occ), pts, J["th"], nnratio=0.8)
        mp[m >= 0] = m[m >= 0]
    searched = mp.copy()
    o = _pose_optimization(f, stereo, mp, tab["pos"], Tcw)
    outlier = np.zeros(n, bool)
    outlier[o.gidx] = o.outlier
    inl = 0
    for i in range(n):  # :1230-1252
        if mp[i] >= 0:
            if not outlier[i]:
                if J["only_tracking"] or flags[mp[i]] & HAS_OBS:
                    inl += 1
            elif J["stereo"]:
                mp[i] = -1
    out.counts.append((inl, 30))
    if J["recently_relocalised"]:
        out.counts.append((inl, 50))
    lost = (J["recently_relocalised"] and inl < 50) or inl < 30
    out.status, out.n_inliers, out.opt, out.Tcw = (LOST if lost else OK), inl, o, o.Tcw
    out.rows, out.point_flags = [searched, mp.copy(), outlier.astype(np.int32)], pf
    return out


def decisive(ref):
    """None when a GPU comparison of this frame is conditioned well, else what fails: every compared count at
    least 3 from the 10, 15, 20, 30 or 50 it is compared with, every classification chi2 at least 1e-6
    (relative) from its threshold."""
    for v, t in ref.counts:
        if abs(v - t) < 3:
            return f"count {v} within 3 of {t}"
    if ref.opt is not None and ref.opt.margin < 1e-6:
        return f"a chi2 within {ref.opt.margin:.3g} of its threshold"
    return None


# ---------------------------------------------------------------- UpdateLastFrame

def unproject_stereo(c, i):
    """Frame::UnprojectStereo (Frame.cpp:787-795): mRwc * x3Dc is a float cv::Mat product (double accumulation,
    rounded once), + mOw a float addition"""
    fx, fy, cx, cy, invfx, invfy = (F32(v) for v in c["K"])
    z = F32(c["depth"][i])
    u, v = F32(c["kps"]["x"][i]), F32(c["kps"]["y"][i])
    x = F32(F32(F32(u - cx) * z) * invfx)
    y = F32(F32(F32(v - cy) * z) * invfy)
    R, Ow = np.asarray(c["Rwc"], F32).reshape(3, 3), np.asarray(c["Ow"], F32)
    with np.errstate(invalid="ignore", over="ignore"):  # an infinite depth gives inf - inf
        return np.array([F32(F32(F64(R[r, 0]) * F64(x) + F64(R[r, 1]) * F64(y) + F64(R[r, 2]) * F64(z)) + Ow[r])
                         for r in range(3)], F32)


def update_last_frame(c):
    """Tracking.cpp:1053-1113, the literal loop.  Returns a dict: created (n,) u8, flags, pos, mp_desc (the slot
    table afterwards), n_created, n_pos, n_visited."""
    n = len(c["depth"])
    flags, pos, mpd = np.array(c["flags"], np.int32), np.array(c["pos"], F32), np.array(c["mp_desc"], np.uint8)
    created = np.zeros(n, np.uint8)
    v_depth_idx = []
    for i in range(n):
        z = F32(c["depth"][i])
        if z > 0:
            v_depth_idx.append((float(z), i))
    visited = 0
    if v_depth_idx:
        v_depth_idx.sort()  # pair<float, int>: by depth, then by index
        n_points = 0
        for z, i in v_depth_idx:
            visited += 1
            create = False
            if not flags[i] & VALID:  # !pMP
                create = True
            elif not flags[i] & HAS_OBS:  # pMP->Observations() < 1
                create = True
            if create:
                pos[i] = unproject_stereo(c, i)
                mpd[i] = c["desc"][i]  # MapPoint(x3D, pMap, pFrame, idx): pFrame->mDescriptors.row(idx)
                flags[i] = (flags[i] | VALID) & ~HAS_OBS
                created[i] = 1
                n_points += 1
            else:
                n_points += 1
            if F32(z) > F32(c["th_depth"]) and n_points > 100:
                break
    return {"created": created, "flags": flags, "pos": pos, "mp_desc": mpd, "n_created": int(created.sum()),
            "n_pos": len(v_depth_idx), "n_visited": visited}


def visited_closed_form(depth, th_depth):
    """the slots the loop visits, by the closed form the kernel uses: the first min(n_pos, max(m, 100) + 1) of
    the (z, i) order, m = the positive depths that are not > th_depth"""
    z = np.asarray(depth, F32)
    with np.errstate(invalid="ignore"):
        pos = z > 0
        m = int((pos & ~(z > F32(th_depth))).sum())
    idx = np.nonzero(pos)[0]
    order = idx[np.lexsort((idx, z[idx]))]
    return order[:min(len(order), max(m, 100) + 1)]
