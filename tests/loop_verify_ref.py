"""CPU restatement of LoopClosing::ComputeSim3's whole candidate loop
(src/LoopClosing.cpp:339-411), verification included: the reference for
csrc/loop_verify.hip.  It composes the oracle's pieces --
loop_ref.Sim3SolverRef (its iterate() is re-callable and keeps its state, and a
return never reports bNoMore), proj_ref.search_by_sim3, OptimizeSim3's gathers
(Optimizer.cpp:1284-1366) and sim3opt_ref.optimize_sim3 -- on a
tests/loop_verify_scene.py scene, drawing from the host glibc rand().

``verify`` is one verification (:358-410) for a given RANSAC Sim3 and inlier
row, so a stage-wise test can feed it the GPU's own Sim3 bits;
``compute_sim3_verified`` is the loop.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import loop_ref
import loop_verify_scene as lvs
import proj_ref
import sim3opt_ref
from lm_ref import quat_from_R

F32 = np.float32


def make_solvers(scene, q, min_matches=20):
    """the Sim3Solvers of query q (None: fewer than 20 BoW matches, :314-318)"""
    cur, cands = scene["queries"][q]
    nc = len(cands)
    out = []
    for c, kf in enumerate(cands):
        p = q * nc + c
        if scene["nmatches"][p] < min_matches:
            out.append(None)
            continue
        corr = loop_ref.sim3_setup(scene["match12"][p], scene["valid"][cur], scene["valid"][kf],
                                   scene["mp_world"][cur], scene["mp_world"][kf], scene["Tcw"][cur], scene["Tcw"][kf],
                                   scene["octave"][cur], scene["octave"][kf], scene["sigma2"])
        out.append(loop_ref.Sim3SolverRef(corr, scene["K"], scene["K"], scene["fix_scale"]))
    return out


def _cam(scene, kf, i):
    R = np.asarray(scene["Tcw"][kf, :9], F32).reshape(3, 3)
    t = np.asarray(scene["Tcw"][kf, 9:], F32)
    return (loop_ref._gemv_f32(R, scene["mp_world"][kf][i]) + t).astype(F32)


def verify(scene, q, c, R12, t12, s12, vb_inliers, th_search=7.5, th2=10.0):
    """SearchBySim3 + OptimizeSim3 of candidate c of query q for the RANSAC Sim3
    (float32 R12, t12, s12) and vbInliers (bool per KF1 slot).  Returns a
    namespace: m_ransac (the row before SearchBySim3), agreed (SearchBySim3's own
    row), n_found, m_search (the row before the removals), gidx (the KF1 slots
    gathered, in order), opt (sim3opt_ref's result), m (the final row), n_in."""
    cur, cands = scene["queries"][q]
    kf = cands[c]
    n1, n2 = len(scene["valid"][cur]), len(scene["valid"][kf])
    row = scene["match12"][q * len(cands) + c]
    vb = np.asarray(vb_inliers, bool)
    m = np.where(vb, row, -1).astype(np.int32)
    out = SimpleNamespace(m_ransac=m.copy())
    v1, v2 = scene["valid"][cur].astype(bool), scene["valid"][kf].astype(bool)
    named = np.zeros(n2, bool)
    named[m[m >= 0]] = True
    f1 = (v1 & (m < 0)).astype(np.int32)
    f2 = (v2 & ~named).astype(np.int32)
    R12 = np.asarray(R12, F32).reshape(3, 3)
    t12 = np.asarray(t12, F32).reshape(3)
    s12 = F32(s12)
    nf, agreed = proj_ref.search_by_sim3(lvs.kf_target(scene, cur), lvs.kf_target(scene, kf),
                                         lvs.kf_points(scene, cur, f1), lvs.kf_points(scene, kf, f2), s12, R12, t12,
                                         th_search)
    out.agreed, out.n_found = agreed, nf
    m[agreed >= 0] = agreed[agreed >= 0]
    out.m_search = m.copy()
    gidx = np.array([i for i in range(n1) if m[i] >= 0 and v1[i] and v2[m[i]]], np.int64)
    out.gidx = gidx
    k1, k2 = scene["kps"][cur], scene["kps"][kf]
    i2 = m[gidx]
    P1c = np.array([_cam(scene, cur, i) for i in gidx], F32).reshape(-1, 3)
    P2c = np.array([_cam(scene, kf, i) for i in i2], F32).reshape(-1, 3)
    obs1 = np.stack([k1["x"][gidx], k1["y"][gidx]], 1).astype(F32).reshape(-1, 2)
    obs2 = np.stack([k2["x"][i2], k2["y"][i2]], 1).astype(F32).reshape(-1, 2)
    w1 = scene["inv_level_sigma2"][k1["octave"][gidx]]
    w2 = scene["inv_level_sigma2"][k2["octave"][i2]]
    # gScm = Sim3(toMatrix3d(R), toVector3d(t), s): Quaterniond(Matrix3d), not normalised
    q12 = quat_from_R([[float(R12[i, j]) for j in range(3)] for i in range(3)])
    opt = sim3opt_ref.optimize_sim3(q12, [float(v) for v in t12], float(s12), P1c, P2c, obs1, obs2, w1, w2,
                                    scene["K"], scene["K"], th2, scene["fix_scale"])
    out.opt = opt
    m[gidx[opt.removed]] = -1
    out.m = m
    out.n_in = opt.n_in
    return out


def scw(scene, kf, S):
    """mg2oScw = gScm * Sim3(Rcw2, tcw2, 1.0) (:402-405): ((q, t, s), float32 4x4)"""
    R = np.asarray(scene["Tcw"][kf, :9], F32).reshape(3, 3)
    t = np.asarray(scene["Tcw"][kf, 9:], F32)
    gSmw = (quat_from_R([[float(R[i, j]) for j in range(3)] for i in range(3)]), [float(v) for v in t], 1.0)
    g = sim3opt_ref.sim3_mul(S, gSmw)
    return g, sim3opt_ref.sim3_to_T(g)


def compute_sim3_verified(scene, q, seed, iterations_per_call=5, min_opt_inliers=20, th_search=7.5,
                          max_verifications=None):
    """The loop from srand(seed); with max_verifications it stops (status
    'pending') after that many verifications have failed.  Returns a dict: status ('matched' /
    'no_match'), matched, round, verifications (list of dicts: cand, round,
    pose, n_inliers, mask, v = verify's namespace), hypotheses, solvers,
    discarded, after (the next rand() of the stream), Scw / Scw_T when matched."""
    solvers = make_solvers(scene, q)
    loop_ref.libc().srand(seed)
    discarded = [s is None for s in solvers]
    n_cand = sum(not d for d in discarded)
    log = []
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
            found, no_more, nin = s.iterate(iterations_per_call)
            if no_more:
                discarded[i] = True
                n_cand -= 1
            if found:
                pose = s.best_pose
                vb = np.zeros(len(scene["valid"][scene["queries"][q][0]]), bool)
                vb[s.idx[s.best_mask]] = True
                v = verify(scene, q, i, pose["R12"], pose["t12"], pose["s12"], vb, th_search=th_search)
                log.append({"cand": i, "round": rnd, "pose": pose, "n_inliers": nin, "vb": vb, "v": v,
                            "iterations": s.iterations, "call_iterations": s.iterations - before,
                            "max_its": s.max_its})
                if v.n_in >= min_opt_inliers:
                    g, T = scw(scene, scene["queries"][q][1][i], v.opt.S)
                    res.update(status="matched", matched=i, round=rnd, Scw=g, Scw_T=T)
                    break
    res["verifications"] = log
    res["hypotheses"] = sum(s.iterations for s in solvers if s is not None)
    res["solvers"], res["discarded"] = solvers, discarded
    res["after"] = loop_ref.libc().rand()
    return res
