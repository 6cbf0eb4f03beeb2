"""CPU restatement of Tracking::Relocalization's candidate loop
(src/Tracking.cpp:1778-1912), verification included: the reference for
csrc/reloc.hip.  It composes the oracle's pieces -- pnp_ref.ransac_call with
draws from the host glibc rand() (as tests/test_pnp.py), poseopt_ref's
PoseOptimization, proj_ref's KEYFRAME SearchByProjection -- on a
tests/reloc_scene.py scene, whose SearchByBoW rows are bow_ref's.

``verify`` is one verification (:1832-1899) for a given PnP pose and inlier
row, optionally with the pose each optimisation left injected, so a stage-wise
test can feed it the GPU's own bits; ``relocalize`` is the loop and logs every
iterate() call and every verification.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import loop_ref
import pnp_ref
import poseopt_ref
import proj_ref
import reloc_scene as rs

F32 = np.float32
MIN_MATCHES = 15


class PnPSolverRef:
    """PnPsolver(F, vpMapPointMatches) + SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    (PnPsolver.cpp:104-195); iterate() is re-callable and keeps its state."""

    def __init__(self, scene, q, c):
        f, kfs = scene["queries"][q]
        kf = kfs[c]
        row = scene["match"][q * len(kfs) + c]
        k = scene["f_kps"][f]
        idx = [j for j in range(len(row)) if row[j] >= 0 and scene["valid"][kf][row[j]]]  # pMP && !pMP->isBad()
        self.kidx = np.array(idx, np.int64)  # mvKeyPointIndices
        self.P2 = np.stack([k["x"][idx], k["y"][idx]], 1).astype(F32).reshape(-1, 2)
        self.P3w = scene["mp_world"][kf][row[idx]].astype(F32).reshape(-1, 3)
        self.maxerr = (scene["sigma2"][k["octave"][idx]] * F32(5.991)).astype(F32)  # mvMaxError
        self.cam = tuple(float(v) for v in scene["K"])
        self.n_matches = len(row)
        N = self.N = len(idx)
        eps = F32(0.5)
        n_min = max(int(F32(N) * eps), 10, 4)  # int nMinInliers = N * mRansacEpsilon, then the two floors
        self.min_inliers = n_min
        with np.errstate(all="ignore"):
            if eps < F32(n_min) / F32(N):
                eps = F32(n_min) / F32(N)
            if n_min == N:
                n_it = 1
            else:
                e3 = float(eps) ** 3
                v = math.log(1 - 0.99) / math.log(1 - e3) if 0 < e3 < 1 else float("nan")
                n_it = int(math.ceil(v)) if math.isfinite(v) and abs(v) < 2 ** 31 else -(2 ** 31)
        self.max_its = max(1, min(n_it, 300))
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(N, bool)
        self.best_Tcw = None
        self.min_count_gap = 10 ** 9   # decisiveness: the closest an inlier count came to min_inliers
        self.min_err_gap = float("inf")  # and a reprojection error to its mvMaxError (relative)

    def _watch(self, R, t):
        if R is None:
            return
        fu, fv, uc, vc = self.cam
        X = self.P3w.astype(np.float64)
        Xc = X @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
        with np.errstate(all="ignore"):
            e2 = (self.P2[:, 0] - (uc + fu * Xc[:, 0] / Xc[:, 2])) ** 2 + (self.P2[:, 1] - (vc + fv * Xc[:, 1] / Xc[:, 2])) ** 2
            gap = np.abs(e2 - self.maxerr) / self.maxerr
        if np.isfinite(gap).any():
            self.min_err_gap = min(self.min_err_gap, float(np.nanmin(gap)))

    def iterate(self, n_iterations, draw):
        """PnPsolver::iterate (:203-301).  draw(n, n_iter) -> (n_iter, 4) minimal sets and a commit(consumed)
        that leaves the stream after exactly the consumed iterations.  Returns (Tcw or None, bNoMore,
        vbInliers, nInliers, refined)."""
        vb = np.zeros(self.n_matches, bool)
        if self.N < self.min_inliers:
            return None, True, vb, 0, False
        n_hyp = max(self.max_its - self.iterations, n_iterations)  # the `||` of :224
        samples, commit = draw(self.N, n_hyp)
        r = pnp_ref.ransac_call(self.P3w, self.P2, self.maxerr, self.cam, self.min_inliers, self.best_inliers,
                                self.best_mask, samples)
        commit(r["consumed"])
        pw, us = self.P3w.astype(np.float64), self.P2.astype(np.float64)
        for idx in samples[:r["consumed"]]:  # decisiveness: every hypothesis' count against min_inliers
            R, t, _ = pnp_ref.compute_pose(pw[idx], us[idx], self.cam)
            cnt = int(pnp_ref.check_inliers(R, t, self.P3w, self.P2, self.maxerr, self.cam).sum())
            self.min_count_gap = min(self.min_count_gap, abs(cnt - self.min_inliers))
            self._watch(R, np.asarray(t).reshape(3))
        self.iterations += r["consumed"]
        self.last_consumed = r["consumed"]
        self.best_inliers = r["best_inliers"]
        if r["best_hyp"] >= 0:
            self.best_mask = r["best_mask"].copy()
            T = np.eye(4, dtype=F32)
            T[:3, :3], T[:3, 3] = r["best_R"].astype(F32), np.asarray(r["best_t"]).reshape(3).astype(F32)
            self.best_Tcw = T
            self.min_count_gap = min(self.min_count_gap, abs(r["best_inliers"] - self.min_inliers))
            self._watch(r["best_R"], np.asarray(r["best_t"]).reshape(3))
        if r["refined_mask"] is not None:
            self.min_count_gap = min(self.min_count_gap, abs(int(np.sum(r["refined_mask"])) - self.min_inliers))
            self._watch(r["refined_R"], np.asarray(r["refined_t"]).reshape(3))
        if r["found"]:
            vb[self.kidx[r["refined_mask"].astype(bool)]] = True
            T = np.eye(4, dtype=F32)
            T[:3, :3], T[:3, 3] = r["refined_R"].astype(F32), np.asarray(r["refined_t"]).reshape(3).astype(F32)
            return T, False, vb, r["refined_inliers"], True
        no_more = self.iterations >= self.max_its
        if no_more and self.best_inliers >= self.min_inliers:
            vb[self.kidx[self.best_mask]] = True
            return self.best_Tcw.copy(), True, vb, self.best_inliers, False
        return None, no_more, vb, 0, False


def make_solvers(scene, q):
    """the PnPsolvers of query q (None: fewer than 15 BoW matches, :1787-1791)"""
    nc = len(scene["queries"][q][1])
    return [PnPSolverRef(scene, q, c) if scene["nmatches"][q * nc + c] >= MIN_MATCHES else None for c in range(nc)]


def _pose_optimization(scene, f, kf, mp, Tcw, outlier):
    """Optimizer::PoseOptimization(&mCurrentFrame): the gather over the keypoints with a MapPoint, mvbOutlier
    written where one is present, the pose set.  Returns poseopt_ref's namespace plus gidx and margin."""
    k = scene["f_kps"][f]
    gidx = np.nonzero(mp >= 0)[0]
    Xw = scene["mp_world"][kf][mp[gidx]].astype(F32).reshape(-1, 3)
    ur = scene["f_uright"][f][gidx] if scene["f_uright"] is not None else np.full(len(gidx), -1.0, F32)
    obs = np.stack([k["x"][gidx], k["y"][gidx], ur], 1).astype(F32).reshape(-1, 3)
    w = scene["inv_level_sigma2"][k["octave"][gidx]]
    o = poseopt_ref.pose_optimization(np.asarray(Tcw, F32)[:3], Xw, obs, w, scene["K"], scene["bf"])
    outlier[gidx] = o.outlier
    o.gidx = gidx
    o.margin = poseopt_ref.threshold_margin(o, obs)
    return o


def _search(scene, f, kf, mp, found, Tcw, th, orb_dist):
    """matcher2.SearchByProjection(mCurrentFrame, pKF, sFound, th, ORBdist), matcher2 = ORBmatcher(0.9, true)"""
    flags = (scene["valid"][kf].astype(bool) & ~found).astype(np.int32)
    tgt = rs.frame_target(scene, f, Tcw, (mp >= 0).astype(np.uint8))
    return proj_ref.search_by_projection(proj_ref.KEYFRAME, tgt, rs.kf_points(scene, kf, flags), th, nnratio=0.9,
                                         check_ori=True, orb_dist=orb_dist)


def verify(scene, q, c, Tcw_pnp, vb_inliers, outlier, stage_poses=None):
    """Tracking.cpp:1832-1899 for candidate c of query q, the PnP pose (float32 4x4) and vbInliers (bool per
    frame keypoint).  outlier: mvbOutlier (bool per frame keypoint), updated in place.  stage_poses: {1, 2, 3:
    4x4} replaces the pose an optimisation left before anything reads it.  Returns a namespace: vb, opt
    (the optimisations run), rows (mvpMapPoints after each stage; stages not run repeat the row before),
    nadditional [2] (-1: not run), n_good, Tcw, matched."""
    stage_poses = stage_poses or {}
    f, kfs = scene["queries"][q]
    kf = kfs[c]
    row = scene["match"][q * len(kfs) + c]
    vb = np.asarray(vb_inliers, bool)
    mp = np.where(vb, row, -1).astype(np.int32)  # every mvpMapPoints[j] is rewritten (:1840-1849)
    found = np.zeros(len(scene["valid"][kf]), bool)
    found[mp[mp >= 0]] = True
    out = SimpleNamespace(vb=vb.copy(), opt=[], nadditional=[-1, -1], sums=[])
    o = _pose_optimization(scene, f, kf, mp, Tcw_pnp, outlier)
    out.opt.append(o)
    T = np.asarray(stage_poses.get(1, o.Tcw), F32)
    n_good = o.n_good
    rows = []
    if n_good >= 10:
        mp[outlier] = -1  # :1857-1859; sFound keeps the culled points
        rows.append(mp.copy())
        if n_good < 50:
            nadd, m = _search(scene, f, kf, mp, found, T, 10.0, 100)
            out.nadditional[0] = nadd
            mp[m >= 0] = m[m >= 0]
            out.sums.append(nadd + n_good)
            if nadd + n_good >= 50:
                o = _pose_optimization(scene, f, kf, mp, T, outlier)
                out.opt.append(o)
                T = np.asarray(stage_poses.get(2, o.Tcw), F32)
                n_good = o.n_good
                rows.append(mp.copy())  # the outliers of this optimisation keep their MapPoints
                if 30 < n_good < 50:
                    found[:] = False
                    found[mp[mp >= 0]] = True
                    nadd, m = _search(scene, f, kf, mp, found, T, 3.0, 64)
                    out.nadditional[1] = nadd
                    mp[m >= 0] = m[m >= 0]
                    out.sums.append(nadd + n_good)
                    if n_good + nadd >= 50:
                        o = _pose_optimization(scene, f, kf, mp, T, outlier)
                        out.opt.append(o)
                        T = np.asarray(stage_poses.get(3, o.Tcw), F32)
                        n_good = o.n_good
                        mp[outlier] = -1
    else:
        rows.append(mp.copy())
    while len(rows) < 2:
        rows.append(rows[-1].copy())
    rows.append(mp.copy())
    out.rows = rows[:3]
    out.n_good, out.Tcw, out.matched = n_good, T, n_good >= 50
    out.n_goods = [x.n_good for x in out.opt]
    return out


class HostStream:
    """the host glibc stream from srand(seed), with the draws of an iterate() call laid out ahead and the
    stream then left after exactly the consumed ones"""

    def __init__(self, seed):
        self.seed, self.used = seed, 0
        loop_ref.libc().srand(seed)

    def draw(self, n, n_iter):
        out = np.zeros((n_iter, 4), np.int32)
        for it in range(n_iter):  # PnPsolver.cpp:230-244
            avail = list(range(n))
            for j in range(4):
                r = loop_ref.random_int(0, len(avail) - 1)
                out[it, j] = avail[r]
                avail[r] = avail[-1]
                avail.pop()

        def commit(consumed):
            self.used += 4 * consumed
            loop_ref.libc().srand(self.seed)
            for _ in range(self.used):
                loop_ref.libc().rand()

        return out, commit


def relocalize(scene, q, seed, max_verifications=None):
    """The loop from srand(seed); with max_verifications it stops (status 'pending') before the iterate()
    call that would follow that many verifications.  Returns a dict: status ('matched' / 'no_match' /
    'pending'), matched, round (of the last iterate() call), calls (list of dicts: cand, round, n_hyp run,
    iterations after, no_more, returned), verifications (list of dicts: cand, round, Tcw, n_inliers,
    refined, vb, v = verify's namespace), hypotheses, solvers, discarded, outlier (mvbOutlier at the end),
    after (the next rand() of the stream)."""
    solvers = make_solvers(scene, q)
    stream = HostStream(seed)
    discarded = [s is None for s in solvers]
    n_cand = sum(not d for d in discarded)
    f = scene["queries"][q][0]
    outlier = np.zeros(len(scene["f_kps"][f]), bool)  # the Frame ctor's mvbOutlier
    calls, log = [], []
    res = {"status": "no_match", "matched": -1, "round": -1}
    rnd = -1
    while n_cand > 0 and res["matched"] < 0 and res["status"] != "pending":
        rnd += 1
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            if max_verifications is not None and len(log) >= max_verifications:
                res["status"] = "pending"
                break
            before = s.iterations
            T, no_more, vb, nin, refined = s.iterate(5, stream.draw)
            res["round"] = rnd
            calls.append({"cand": i, "round": rnd, "before": before, "ran": s.iterations - before,
                          "iterations": s.iterations, "max_its": s.max_its, "no_more": no_more,
                          "returned": T is not None, "refined": refined})
            if no_more:
                discarded[i] = True
                n_cand -= 1
            if T is not None:
                v = verify(scene, q, i, T, vb, outlier)
                log.append({"cand": i, "round": rnd, "Tcw": T, "n_inliers": nin, "refined": refined, "vb": vb, "v": v,
                            "no_more": no_more})
                if v.matched:
                    res.update(status="matched", matched=i)
                    break
    res["calls"], res["verifications"] = calls, log
    res["hypotheses"] = sum(s.iterations for s in solvers if s is not None)
    res["solvers"], res["discarded"], res["outlier"] = solvers, discarded, outlier
    res["after"] = loop_ref.libc().rand()
    return res


def decisive(ref):
    """The conditions of a GPU comparison, on the reference (None when they hold, else what fails): every
    nGood and every sum compared with 10, 30 or 50 at least 3 away from it; every PnP inlier count compared
    with min_inliers further from it than test_pnp.py's mask cap max(1, N // 100); every classification chi2
    of every optimisation at least 1e-6 (relative) from its threshold; no PnP reprojection error within a
    relative 1e-3 of its mvMaxError."""
    for s in ref["solvers"]:
        if s is None or s.N < s.min_inliers:
            continue
        if s.min_count_gap <= max(1, s.N // 100):
            return f"a PnP inlier count {s.min_count_gap} from min_inliers (N = {s.N})"
        if s.min_err_gap < 1e-3:
            return f"a PnP reprojection error within {s.min_err_gap:.3g} of its bound"
    for e in ref["verifications"]:
        v = e["v"]
        for k, o in enumerate(v.opt):
            ths = (10, 50) if k == 0 else (30, 50) if k == 1 else (50,)
            if any(abs(o.n_good - t) < 3 for t in ths):
                return f"nGood {o.n_good} of optimisation {k + 1} within 3 of a threshold"
            if o.margin < 1e-6:
                return f"a chi2 within {o.margin:.3g} of its threshold"
        if any(abs(sm - 50) < 3 for sm in v.sums):
            return f"a sum {v.sums} within 3 of 50"
    return None
