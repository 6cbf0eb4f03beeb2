"""Scenes for the verified loop of LoopClosing::ComputeSim3 (csrc/loop_verify.hip,
tests/loop_verify_ref.py): a synth.loop_burst_scene burst whose keyframes also
carry what SearchBySim3 and OptimizeSim3 read -- keypoints (the projection of
each slot's camera point plus sub-pixel noise, the scene's octave), image
bounds, the scale pyramid, and per MapPoint a descriptor (its keypoint's) and
the distance invariance range as synth.sim3_search_scenario makes it.

One more candidate type, the *decoy*, passes RANSAC and fails verification:
the MapPoints it shares with the current keyframe agree with it under the
candidate's Sim3 exactly (no 3D noise), so iterate() returns at once with
every correspondence an inlier; its keypoints at those slots are displaced by
DECOY_PX pixels (many sigma at any level) from the projections, so every
correspondence fails OptimizeSim3's chi2 check in the candidate's image.

``match12`` rows come from the CPU oracle (bow_ref.search_by_bow over a small
vocabulary), optionally thinned to the first `keep` true pairs of a candidate.
"""
from __future__ import annotations

import functools

import numpy as np

import bow_ref
import loop_ref
import orbgpu
import synth

DECOY_PX = 40.0
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LOG_SF = float(np.log(np.float32(1.2)))


@functools.lru_cache(maxsize=None)
def vocabulary():
    k, L = 10, 4
    p, l, d, w = synth.synthetic_vocabulary_fast(k, L, 5)
    return loop_ref.ArrayVocabulary(k, L, 0, 0, p, l, d, w), d[l == 1]


def cam_points(scene, kf):
    R = scene["Tcw"][kf, :9].reshape(3, 3).astype(np.float64)
    t = scene["Tcw"][kf, 9:].astype(np.float64)
    return scene["mp_world"][kf].astype(np.float64) @ R.T + t


def build(n_queries, n_cand, n_kp=300, inlier_frac=0.4, outlier_frac=0.0, decoys=(), seed=1, fix_scale=False,
          keep=None, kp_noise=0.3, leaves=None, oracle_bow=True):
    """decoys: candidate slots (0..n_cand-1) that are decoys in every query.
    keep: {candidate slot: n}: that candidate's match12 row keeps only its
    first n true pairs (everything else -1).  Returns the scene dict of
    synth.loop_burst_scene plus kps, mp_desc, min_dist, max_dist,
    inv_level_sigma2, queries [(cur, [cands])], match12 / nmatches per pair.
    leaves: the vocabulary leaves the descriptors start from (default: the small
    vocabulary's); oracle_bow=False leaves match12 / nmatches out (a caller with
    a vocabulary on the GPU runs SearchByBoW there)."""
    if leaves is None:
        avoc, leaves = vocabulary()
    scene = synth.loop_burst_scene(n_queries, n_cand, leaves, n_kp=n_kp, inlier_frac=inlier_frac,
                                   outlier_frac=outlier_frac, seed=seed, fix_scale=fix_scale)
    rng = np.random.default_rng(seed + 0x5EED)
    K = scene["K"].astype(np.float64)
    n_kf = len(scene["desc"])
    # decoys: exact 3D agreement under the candidate's Sim3
    for q in range(n_queries):
        X1c = cam_points(scene, q)
        for c in decoys:
            kf = n_queries + q * n_cand + c
            tr = scene["truth"][q * n_cand + c]
            Y = ((X1c[tr["src"]] - tr["t"]) @ tr["R"]) / tr["s"]
            R2 = scene["Tcw"][kf, :9].reshape(3, 3).astype(np.float64)
            t2 = scene["Tcw"][kf, 9:].astype(np.float64)
            scene["mp_world"][kf, tr["dst"]] = ((Y - t2) @ R2).astype(np.float32)
    kps = np.zeros((n_kf, n_kp), orbgpu.KP_DTYPE)
    min_dist = np.zeros((n_kf, n_kp), np.float32)
    max_dist = np.zeros((n_kf, n_kp), np.float32)
    for kf in range(n_kf):
        Xc = cam_points(scene, kf)
        z = np.maximum(Xc[:, 2], 1e-3)
        u = K[0] * Xc[:, 0] / z + K[2] + rng.normal(scale=kp_noise, size=n_kp)
        v = K[1] * Xc[:, 1] / z + K[3] + rng.normal(scale=kp_noise, size=n_kp)
        lv = scene["octave"][kf]
        kps[kf]["x"], kps[kf]["y"] = u, v
        kps[kf]["size"] = 31 * SF[lv]
        kps[kf]["angle"] = scene["angle"][kf]
        kps[kf]["octave"] = lv
        kps[kf]["class_id"] = -1
        d = np.linalg.norm(Xc, axis=1)
        maxd = (d * rng.uniform(0.95, 1.05, n_kp) * SF[lv]).astype(np.float32)
        max_dist[kf] = maxd
        min_dist[kf] = maxd / SF[7]
    for q in range(n_queries):
        for c in decoys:
            kf = n_queries + q * n_cand + c
            dst = scene["truth"][q * n_cand + c]["dst"]
            a = rng.uniform(0, 2 * np.pi, len(dst))
            kps[kf]["x"][dst] += (DECOY_PX * np.cos(a)).astype(np.float32)
            kps[kf]["y"][dst] += (DECOY_PX * np.sin(a)).astype(np.float32)
    scene["kps"] = kps
    scene["mp_desc"] = scene["desc"].copy()
    scene["min_dist"], scene["max_dist"] = min_dist, max_dist
    scene["inv_level_sigma2"] = (np.float32(1.0) / scene["sigma2"]).astype(np.float32)
    scene["fix_scale"] = fix_scale
    scene["queries"] = [(q, [n_queries + q * n_cand + c for c in range(n_cand)]) for q in range(n_queries)]
    if not oracle_bow:
        return scene
    # SearchByBoW(mpCurrentKF, pKF) on the CPU oracle
    fvs = {}

    def fv(kf):
        if kf not in fvs:
            fvs[kf] = avoc.transform(scene["desc"][kf], 4)[3]
        return fvs[kf]

    match12 = np.full((n_queries * n_cand, n_kp), -1, np.int32)
    nmatches = np.zeros(n_queries * n_cand, np.int32)
    for q, (cur, cands) in enumerate(scene["queries"]):
        for c, kf in enumerate(cands):
            nm, m12 = bow_ref.search_by_bow(1, fv(cur), scene["desc"][cur], scene["angle"][cur], scene["valid"][cur],
                                            fv(kf), scene["desc"][kf], scene["angle"][kf], scene["valid"][kf],
                                            nnratio=0.75, check_ori=True)
            m12 = np.asarray(m12, np.int32)
            if keep and c in keep:
                tr = scene["truth"][q * n_cand + c]
                true = dict(zip(tr["src"].tolist(), tr["dst"].tolist()))
                good = [i for i in range(n_kp) if m12[i] >= 0 and true.get(i) == m12[i]][:keep[c]]
                thin = np.full(n_kp, -1, np.int32)
                thin[good] = m12[good]
                m12, nm = thin, len(good)
            match12[q * n_cand + c], nmatches[q * n_cand + c] = m12, nm
    scene["match12"], scene["nmatches"] = match12, nmatches
    for v in scene.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return scene


def kf_target(scene, kf):
    """keyframe `kf` as a proj_ref / proj.py target dict"""
    K = scene["K"]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = scene["Tcw"][kf, :9].reshape(3, 3)
    T[:3, 3] = scene["Tcw"][kf, 9:]
    return {"kps": scene["kps"][kf], "desc": scene["desc"][kf], "u_right": None, "occupied": None,
            "min_x": BOUNDS[0], "max_x": BOUNDS[1], "min_y": BOUNDS[2], "max_y": BOUNDS[3], "fx": K[0], "fy": K[1],
            "cx": K[2], "cy": K[3], "bf": 0.0, "b": 0.0, "n_levels": 8, "log_scale_factor": LOG_SF,
            "scale_factors": SF, "Tcw": T}


def kf_points(scene, kf, flags):
    return {"flags": np.asarray(flags, np.int32), "pos": scene["mp_world"][kf], "desc": scene["mp_desc"][kf],
            "min_dist": scene["min_dist"][kf], "max_dist": scene["max_dist"][kf]}
