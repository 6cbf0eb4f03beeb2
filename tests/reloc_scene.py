"""Scenes for Tracking::Relocalization's candidate loop (csrc/reloc.hip,
tests/reloc_ref.py): lost frames, each with candidate keyframes, in the manner
of loop_verify_scene.py -- 300 keypoints, the small vocabulary.

A frame has a true pose and one world point behind every keypoint.  A candidate
keyframe is a list of *groups* of MapPoint slots tied to frame keypoints; every
other slot is unrelated (random descriptor, random MapPoint).  A group is a dict:

  n          slots in the group
  row        True: its pairs may enter SearchByBoW's row (the row is the CPU
             oracle's, bow_ref.search_by_bow, thinned to the true pairs of such
             groups); False: *hidden* -- only the projection searches can find it
  bin        rotation-histogram bin of (keyframe angle - frame angle): 12 deg each
  garbage    the MapPoint is unrelated to the keypoint (a geometric outlier)
  shift_px   the MapPoint projects that many pixels away from its keypoint under
             the true pose: found by a th = 10 search, an outlier of the
             optimisation that follows
  depth      the MapPoint lies at depth * the true depth on the keypoint's ray:
             PnP cannot tell, a stereo observation (mvuRight) can
  keep       at most this many of the group's pairs stay in the row
  invalidate that many of the group's row pairs lose their MapPoint after
             SearchByBoW (isBad by the time the PnPsolver is built)

The rotation bins let a scene steer the searches: the rotation check of
SearchByProjection keeps the three fullest bins of one call, so a small hidden
group in a fourth bin is dropped by the first search and found by the second,
whose only matches it then is.
"""
from __future__ import annotations

import functools

import numpy as np

import bow_ref
import loop_ref
import orbgpu
import synth

BOUNDS = (0.0, 640.0, 0.0, 480.0)
SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LOG_SF = float(np.log(np.float32(1.2)))
K = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
BF = 80.0
N_KP = 300


@functools.lru_cache(maxsize=None)
def vocabulary():
    k, L = 10, 4
    p, l, d, w = synth.synthetic_vocabulary_fast(k, L, 5)
    return loop_ref.ArrayVocabulary(k, L, 0, 0, p, l, d, w), d[l == 1]


def _jitter(rng, d, p):
    bits = np.unpackbits(d, axis=-1)
    m = (rng.random(bits.shape) < p).astype(np.uint8)
    return np.packbits(bits ^ m, axis=-1)


def _back(u, v, z):
    return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], -1)


def build(cands, seed, stereo=False, n_queries=3, n_kp=N_KP, kp_noise=0.2, keep_by_query=None, leaves=None,
          oracle_bow=True):
    """cands: per candidate slot the list of groups (the same layout in every
    query, fresh random data per query).  keep_by_query: {candidate slot: [n per
    query]} overrides the `keep` of that candidate's first group.  leaves: the
    vocabulary leaves the descriptors start from (default: the small
    vocabulary's); oracle_bow=False leaves match / nmatches out (a caller with a
    vocabulary on the GPU runs SearchByBoW there; nothing is thinned or
    invalidated then).  Returns a dict: frame arrays (f_kps,
    f_desc, f_uright or None), keyframe arrays in
    loop.Keyframes / loop.KeyframeSearch order (desc, angle, octave, valid,
    mp_world, Tcw, kps, mp_desc, min_dist, max_dist), K, sigma2,
    inv_level_sigma2, queries [(frame, [kfs])], match / nmatches per pair."""
    if leaves is None:
        avoc, leaves = vocabulary()
    rng = np.random.default_rng(seed)
    nq, nc = n_queries, len(cands)
    n_kf = nq * nc
    sig2 = synth.level_sigma2()
    f_kps = np.zeros((nq, n_kp), orbgpu.KP_DTYPE)
    f_desc = np.zeros((nq, n_kp, 32), np.uint8)
    f_ur = np.full((nq, n_kp), -1.0, np.float32)
    desc = np.zeros((n_kf, n_kp, 32), np.uint8)
    angle = np.zeros((n_kf, n_kp), np.float32)
    octave = np.zeros((n_kf, n_kp), np.int32)
    valid = np.zeros((n_kf, n_kp), np.uint8)
    mp = np.zeros((n_kf, n_kp, 3), np.float32)
    Tcw = np.zeros((n_kf, 12), np.float32)
    kps = np.zeros((n_kf, n_kp), orbgpu.KP_DTYPE)
    min_dist = np.zeros((n_kf, n_kp), np.float32)
    max_dist = np.zeros((n_kf, n_kp), np.float32)
    match = np.full((n_kf, n_kp), -1, np.int32)
    nmatches = np.zeros(n_kf, np.int32)
    for q in range(nq):
        Rf, tf = synth._rot(rng, 0.3), rng.uniform(-1, 1, 3)
        Cf = -Rf.T @ tf
        u, v = rng.uniform(30, 610, n_kp), rng.uniform(30, 450, n_kp)
        z = rng.uniform(3.0, 6.0, n_kp)
        Xw = (_back(u, v, z) - tf) @ Rf  # R^T (Xc - t)
        f_oct = rng.integers(0, 4, n_kp)
        f_kps[q]["x"] = u + rng.normal(scale=kp_noise, size=n_kp)
        f_kps[q]["y"] = v + rng.normal(scale=kp_noise, size=n_kp)
        f_kps[q]["size"] = 31 * SF[f_oct]
        f_kps[q]["angle"] = rng.uniform(0, 360, n_kp)
        f_kps[q]["octave"] = f_oct
        f_kps[q]["class_id"] = -1
        f_desc[q] = _jitter(rng, leaves[rng.integers(0, len(leaves), n_kp)], 0.08)
        if stereo:
            f_ur[q] = (f_kps[q]["x"] - BF / z).astype(np.float32)
        fv_f = avoc.transform(f_desc[q], 4)[3] if oracle_bow else None
        for c, groups in enumerate(cands):
            kf = q * nc + c
            Rk, tk = synth._rot(rng, 0.1) @ Rf, tf + rng.uniform(-0.3, 0.3, 3)
            Tcw[kf, :9], Tcw[kf, 9:] = Rk.astype(np.float32).ravel(), tk.astype(np.float32)
            # unrelated slots
            desc[kf] = _jitter(rng, leaves[rng.integers(0, len(leaves), n_kp)], 0.08)
            angle[kf] = rng.uniform(0, 360, n_kp)
            octave[kf] = rng.integers(0, 4, n_kp)
            valid[kf] = rng.random(n_kp) < 0.9
            Xk = (_back(rng.uniform(10, 630, n_kp), rng.uniform(10, 470, n_kp), rng.uniform(3, 6, n_kp)) - tk) @ Rk
            total = sum(g["n"] for g in groups)
            src_all = rng.choice(n_kp, total, replace=False)
            dst_all = rng.choice(n_kp, total, replace=False)
            row_pairs, o = {}, 0
            for gi, g in enumerate(groups):
                src, dst = src_all[o:o + g["n"]], dst_all[o:o + g["n"]]
                o += g["n"]
                if not g.get("garbage"):
                    X = Xw[src]
                    if g.get("shift_px"):
                        a = rng.uniform(0, 2 * np.pi, g["n"])
                        X = (_back(u[src] + g["shift_px"] * np.cos(a), v[src] + g["shift_px"] * np.sin(a), z[src]) - tf) @ Rf
                    if g.get("depth"):
                        X = Cf + g["depth"] * (X - Cf)
                    Xk[dst] = X
                desc[kf, dst] = _jitter(rng, f_desc[q, src], 0.03)
                angle[kf, dst] = np.mod(f_kps[q]["angle"][src] + np.float32(12.0 * g.get("bin", 0)), 360.0)
                octave[kf, dst] = f_oct[src]
                valid[kf, dst] = 1
                if g.get("row", False):
                    for s, d in zip(src.tolist(), dst.tolist()):
                        row_pairs[s] = (d, gi)
            mp[kf] = Xk.astype(np.float32)
            # the keyframe's own keypoints and the distance range of its MapPoints: PredictScale in the
            # frame gives a tied slot its keypoint's octave
            Xc = Xk @ Rk.T + tk
            zk = np.maximum(Xc[:, 2], 1e-3)
            kps[kf]["x"] = K[0] * Xc[:, 0] / zk + K[2]
            kps[kf]["y"] = K[1] * Xc[:, 1] / zk + K[3]
            kps[kf]["size"] = 31 * SF[octave[kf]]
            kps[kf]["angle"] = angle[kf]
            kps[kf]["octave"] = octave[kf]
            kps[kf]["class_id"] = -1
            dist = np.linalg.norm(Xk - Cf, axis=1)
            max_dist[kf] = (dist * SF[octave[kf]] * 0.95).astype(np.float32)
            min_dist[kf] = max_dist[kf] / SF[7]
            if not oracle_bow:
                continue
            # SearchByBoW(pKF, F) on the CPU oracle, thinned to the true pairs of the row groups
            fv_k = avoc.transform(desc[kf], 4)[3]
            nm, m = bow_ref.search_by_bow(0, fv_k, desc[kf], angle[kf], valid[kf], fv_f, f_desc[q],
                                          f_kps[q]["angle"], np.ones(n_kp, np.uint8), nnratio=0.75, check_ori=True)
            kept = {gi: 0 for gi in range(len(groups))}
            thin = np.full(n_kp, -1, np.int32)
            for j in range(n_kp):
                if m[j] >= 0 and j in row_pairs and row_pairs[j][0] == m[j]:
                    gi = row_pairs[j][1]
                    limit = groups[gi].get("keep", n_kp)
                    if keep_by_query and c in keep_by_query and gi == 0:
                        limit = keep_by_query[c][q]
                    if kept[gi] < limit:
                        thin[j] = m[j]
                        kept[gi] += 1
            match[kf], nmatches[kf] = thin, int((thin >= 0).sum())
            for gi, g in enumerate(groups):  # MapPoints gone bad between SearchByBoW and the PnPsolver
                if g.get("invalidate"):
                    js = [j for j in range(n_kp) if thin[j] >= 0 and row_pairs[j][1] == gi][:g["invalidate"]]
                    valid[kf, thin[js]] = 0
    scene = {"f_kps": f_kps, "f_desc": f_desc, "f_uright": f_ur if stereo else None, "desc": desc,
             "angle": angle, "octave": octave, "valid": valid, "mp_world": mp, "Tcw": Tcw, "kps": kps,
             "mp_desc": desc.copy(), "min_dist": min_dist, "max_dist": max_dist, "K": K, "bf": BF if stereo else 0.0,
             "sigma2": sig2, "inv_level_sigma2": (np.float32(1.0) / sig2).astype(np.float32),
             "queries": [(q, [q * nc + c for c in range(nc)]) for q in range(nq)], "n_cand": nc}
    if oracle_bow:
        scene["match"], scene["nmatches"] = match, nmatches
    for val in scene.values():
        if isinstance(val, np.ndarray):
            val.setflags(write=False)
    return scene


def frame_target(scene, f, Tcw, occupied):
    """frame f at pose Tcw as a proj_ref / proj.py target dict"""
    Kc = scene["K"]
    return {"kps": scene["f_kps"][f], "desc": scene["f_desc"][f],
            "u_right": None if scene["f_uright"] is None else scene["f_uright"][f], "occupied": occupied,
            "min_x": BOUNDS[0], "max_x": BOUNDS[1], "min_y": BOUNDS[2], "max_y": BOUNDS[3], "fx": Kc[0], "fy": Kc[1],
            "cx": Kc[2], "cy": Kc[3], "bf": scene["bf"], "b": 0.0, "n_levels": 8, "log_scale_factor": LOG_SF,
            "scale_factors": SF, "Tcw": np.asarray(Tcw, np.float32).reshape(4, 4)}


def kf_points(scene, kf, flags):
    return {"flags": np.asarray(flags, np.int32), "pos": scene["mp_world"][kf], "desc": scene["mp_desc"][kf],
            "min_dist": scene["min_dist"][kf], "max_dist": scene["max_dist"][kf], "angle": scene["angle"][kf]}
