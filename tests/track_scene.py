"""Scenes for Tracking's per-frame chain (csrc/track.hip, tests/track_ref.py),
in the manner of reloc_scene.py: frames of up to 300 keypoints with a true pose
and one world point behind every keypoint, descriptors of uniform random bits.

Call 1 (``initial_batch``).  A frame's point table (the last frame's slots in
motion mode, the reference keyframe's in reference mode) is a list of *groups*
of slots tied to frame keypoints; every other slot is unrelated (random
descriptor and position).  A group is a dict:

  n          slots in the group
  bin        rotation-histogram bin of (slot angle - keypoint angle), 12 deg each
  shift_px   the point projects that many pixels from its keypoint under the
             true pose (found by the search, an outlier of the optimisation)
  obs        False: the point has no observations (a visual-odometry point)
  at_init    the point projects onto its keypoint under the START pose: the first
             search finds it whatever init_shift_px is, the optimisation culls it
  row        reference mode: False keeps the pair out of SearchByBoW's row

The start pose is the true pose turned about the camera's y axis so that every
projection moves by about ``init_shift_px``: between th and 2*th times the
octave's scale factor, only the retry finds the matches.

Call 2 (``local_batch``).  The table is n_local local points followed by the
frame-held extras.  Groups:

  n          points in the group
  where      "local" / "extra": the part of the table they live in
  held       True: frame_mp of the keypoint names the point
  bad        the point is bad (VALID clear)
  obs        False: no observations
  shift_px   as above
  onto       "free" (default): the keypoint holds nothing; "obs" / "noobs": an
             unheld local point projects onto a keypoint that holds an extra
             point with / without observations
  view       "ok" (default); "cos": the normal is turned so viewCos < 0.5;
             "wide": viewCos just under 0.998 (the 4.0 radius)
"""
from __future__ import annotations

import numpy as np

import orbgpu
import synth
from reloc_scene import BF, BOUNDS, K, LOG_SF, SF

N_KP = 300
VALID, HAS_OBS = 1, 2
SIGMA2 = synth.level_sigma2()
INV_SIGMA2 = (np.float32(1.0) / SIGMA2).astype(np.float32)


def _jitter(rng, d, p):
    bits = np.unpackbits(d, axis=-1)
    m = (rng.random(bits.shape) < p).astype(np.uint8)
    return np.packbits(bits ^ m, axis=-1)


def _back(u, v, z):
    return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], -1)


def _pose(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R.astype(np.float32), t.astype(np.float32)
    return T


def turned(R, t, shift_px):
    """the pose turned about the camera's y axis: projections move by about shift_px"""
    a = shift_px / float(K[0])
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return _pose(Ry @ R, Ry @ t)


def make_frame(rng, n_kp, stereo, octaves, kp_noise):
    R, t = synth._rot(rng, 0.3), rng.uniform(-1, 1, 3)
    u, v = rng.uniform(40, 600, n_kp), rng.uniform(40, 440, n_kp)
    z = rng.uniform(3.0, 6.0, n_kp)
    kps = np.zeros(n_kp, orbgpu.KP_DTYPE)
    octv = rng.integers(octaves[0], octaves[1] + 1, n_kp)
    kps["x"] = u + rng.normal(scale=kp_noise, size=n_kp)
    kps["y"] = v + rng.normal(scale=kp_noise, size=n_kp)
    kps["size"] = 31 * SF[octv]
    kps["angle"] = rng.uniform(0, 360, n_kp)
    kps["octave"] = octv
    kps["class_id"] = -1
    f = {"R": R, "t": t, "C": -R.T @ t, "u": u, "v": v, "z": z, "kps": kps,
         "Xw": (_back(u, v, z) - t) @ R,
         "desc": rng.integers(0, 256, (n_kp, 32), dtype=np.uint8),
         "u_right": (kps["x"] - BF / z).astype(np.float32) if stereo else None, "Tcw": _pose(R, t)}
    return f


def world(f, src, rng, shift_px=0.0):
    """the world points behind keypoints src, moved shift_px in the image"""
    if not shift_px:
        return f["Xw"][src]
    a = rng.uniform(0, 2 * np.pi, len(src))
    return (_back(f["u"][src] + shift_px * np.cos(a), f["v"][src] + shift_px * np.sin(a), f["z"][src]) - f["t"]) @ f["R"]


def random_world(f, rng, n):
    return (_back(rng.uniform(10, 630, n), rng.uniform(10, 470, n), rng.uniform(3, 6, n)) - f["t"]) @ f["R"]


def frame_target(f, stereo, Tcw, occupied):
    """a frame at pose Tcw as a proj_ref / proj.py target dict"""
    return {"kps": f["kps"], "desc": f["desc"], "u_right": f["u_right"], "occupied": occupied,
            "min_x": BOUNDS[0], "max_x": BOUNDS[1], "min_y": BOUNDS[2], "max_y": BOUNDS[3], "fx": K[0], "fy": K[1],
            "cx": K[2], "cy": K[3], "bf": BF if stereo else 0.0, "b": 0.0, "n_levels": 8, "log_scale_factor": LOG_SF,
            "scale_factors": SF, "Tcw": np.asarray(Tcw, np.float32).reshape(4, 4)}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


def initial_batch(specs, seed, stereo=False, n_kp=N_KP, kp_noise=0.2):
    """specs: per frame a dict: mode (0 motion / 1 reference), groups, th, only_tracking, init_shift_px
    (default 2), octaves (lo, hi) (default (0, 3)), n_slots (default n_kp), forward (stereo, motion: the last
    frame lies behind the current one by that much along z).  Returns {"stereo", "frames": [frame dicts],
    "jobs": [dict: mode, frame, mono, th, only_tracking, Tcw_init, last_Tcw, table {flags, pos, desc, octave,
    angle}, bow_row, bow_nmatches, pairs {keypoint: slot}]}."""
    rng = np.random.default_rng(seed)
    frames, jobs = [], []
    for fi, sp in enumerate(specs):
        f = make_frame(rng, n_kp, stereo, sp.get("octaves", (0, 3)), kp_noise)
        ns = sp.get("n_slots", n_kp)
        flags = np.where(rng.random(ns) < 0.9, VALID | HAS_OBS, 0).astype(np.int32)
        pos = random_world(f, rng, ns)
        desc = rng.integers(0, 256, (ns, 32), dtype=np.uint8)
        octave = rng.integers(0, 4, ns).astype(np.int32)
        angle = rng.uniform(0, 360, ns).astype(np.float32)
        total = sum(g["n"] for g in sp["groups"])
        src_all, dst_all = rng.choice(n_kp, total, replace=False), rng.choice(ns, total, replace=False)
        Tinit = turned(f["R"], f["t"], sp.get("init_shift_px", 2.0))
        Ri, ti = Tinit[:3, :3].astype(np.float64), Tinit[:3, 3].astype(np.float64)
        row = np.full(n_kp, -1, np.int32)
        pairs, o = {}, 0
        for g in sp["groups"]:
            src, dst = src_all[o:o + g["n"]], dst_all[o:o + g["n"]]
            o += g["n"]
            pos[dst] = world(f, src, rng, g.get("shift_px", 0.0))
            if g.get("at_init"):
                pos[dst] = (_back(f["u"][src], f["v"][src], f["z"][src]) - ti) @ Ri
            desc[dst] = _jitter(rng, f["desc"][src], 0.03)
            octave[dst] = f["kps"]["octave"][src]
            angle[dst] = np.mod(f["kps"]["angle"][src] + np.float32(12.0 * g.get("bin", 0)), 360.0)
            flags[dst] = VALID | (HAS_OBS if g.get("obs", True) else 0)
            pairs.update(zip(src.tolist(), dst.tolist()))
            if g.get("row", True):
                row[src] = dst
        mode = sp.get("mode", 0)
        last = _pose(f["R"], f["t"] + np.array([0.0, 0.0, sp.get("forward", 0.0)]))
        jobs.append({"mode": mode, "frame": fi, "mono": int(not stereo), "th": float(sp.get("th", 7 if stereo else 15)),
                     "only_tracking": int(sp.get("only_tracking", 0)), "Tcw_init": Tinit, "last_Tcw": last,
                     "table": {"flags": flags, "pos": pos.astype(np.float32), "desc": desc, "octave": octave,
                               "angle": angle},
                     "bow_row": row if mode == 1 else None, "bow_nmatches": int((row >= 0).sum()) if mode == 1 else None,
                     "pairs": pairs})
        frames.append(f)
    return _freeze({"stereo": stereo, "frames": frames, "jobs": jobs})


def local_batch(specs, seed, stereo=False, n_kp=N_KP, kp_noise=0.2):
    """specs: per frame a dict: groups, n_local, n_extra, th, stereo (the job's flag, default the batch's),
    only_tracking, recently_relocalised, pose_shift_px (default 0.8), octaves.  Returns {"stereo", "frames",
    "jobs": [dict: frame, Tcw, frame_mp, n_local, th, stereo, only_tracking, recently_relocalised, table {flags,
    pos, normal, desc, min_dist, max_dist}, groups {name: (keypoints, points)}]}."""
    rng = np.random.default_rng(seed)
    frames, jobs = [], []
    for fi, sp in enumerate(specs):
        f = make_frame(rng, n_kp, stereo, sp.get("octaves", (0, 3)), kp_noise)
        nl, ne = sp["n_local"], sp.get("n_extra", 0)
        npt = nl + ne
        flags = np.where(rng.random(npt) < 0.9, VALID | HAS_OBS, 0).astype(np.int32)
        pos = random_world(f, rng, npt)
        desc = rng.integers(0, 256, (npt, 32), dtype=np.uint8)
        octv = rng.integers(0, 4, npt)
        view = np.zeros(npt, np.int32)
        frame_mp = np.full(n_kp, -1, np.int32)
        total = sum(g["n"] for g in sp["groups"])
        src_all = rng.choice(n_kp, total, replace=False)
        free_local, free_extra = list(rng.permutation(nl)), list(nl + rng.permutation(ne))
        take = lambda where, n: [(free_local if where == "local" else free_extra).pop() for _ in range(n)]  # noqa: E731
        named, o = {}, 0
        for gi, g in enumerate(sp["groups"]):
            src = src_all[o:o + g["n"]]
            o += g["n"]
            dst = np.array(take(g.get("where", "local"), g["n"]), np.int64)
            pos[dst] = world(f, src, rng, g.get("shift_px", 0.0))
            desc[dst] = _jitter(rng, f["desc"][src], 0.03)
            octv[dst] = f["kps"]["octave"][src]
            flags[dst] = (0 if g.get("bad") else VALID) | (HAS_OBS if g.get("obs", True) else 0)
            view[dst] = {"ok": 0, "cos": 1, "wide": 2}[g.get("view", "ok")]
            if g.get("held"):
                frame_mp[src] = dst
            onto = g.get("onto", "free")
            if onto != "free":  # the keypoint already holds an extra point, with or without observations
                ext = np.array(take("extra", g["n"]), np.int64)
                pos[ext] = world(f, src, rng)
                flags[ext] = VALID | (HAS_OBS if onto == "obs" else 0)
                frame_mp[src] = ext
            named[g.get("name", f"g{gi}")] = (src.copy(), dst.copy())
        # the distance range gives PredictScale the tied keypoint's octave; the normal looks at the camera
        d = pos - f["C"]
        dist = np.linalg.norm(d, axis=1)
        normal = d / dist[:, None]
        for i in np.nonzero(view)[0]:
            a = np.deg2rad(75.0 if view[i] == 1 else 5.0)  # cos 75 < 0.5; 0.5 < cos 5 = 0.9962 < 0.998
            ax = np.cross(normal[i], [0.0, 0.0, 1.0])
            ax /= np.linalg.norm(ax)
            normal[i] = normal[i] * np.cos(a) + np.cross(ax, normal[i]) * np.sin(a)
        max_dist = (dist * SF[octv] * 0.95).astype(np.float32)
        stereo_job = int(sp.get("stereo", stereo))
        jobs.append({"frame": fi, "Tcw": turned(f["R"], f["t"], sp.get("pose_shift_px", 0.8)), "frame_mp": frame_mp,
                     "n_local": nl, "th": float(sp.get("th", 1)), "stereo": stereo_job,
                     "only_tracking": int(sp.get("only_tracking", 0)),
                     "recently_relocalised": int(sp.get("recently_relocalised", 0)),
                     "table": {"flags": flags, "pos": pos.astype(np.float32), "normal": normal.astype(np.float32),
                               "desc": desc, "min_dist": (max_dist / SF[7]).astype(np.float32), "max_dist": max_dist},
                     "groups": named})
        frames.append(f)
    return _freeze({"stereo": stereo, "frames": frames, "jobs": jobs})


def frames_arrays(batch, stride=None, counts=None):
    """the batch's frames as reloc.Frames' arguments (kps, desc, u_right, K, bf, bounds, scale_factors,
    level_sigma2, inv_level_sigma2, log_scale_factor, counts), padded to `stride`"""
    fs = batch["frames"]
    S = stride or max(len(f["kps"]) for f in fs)
    kps = np.zeros((len(fs), S), orbgpu.KP_DTYPE)
    desc = np.zeros((len(fs), S, 32), np.uint8)
    ur = np.full((len(fs), S), -1.0, np.float32)
    for i, f in enumerate(fs):
        n = len(f["kps"])
        kps[i, :n], desc[i, :n] = f["kps"], f["desc"]
        if batch["stereo"]:
            ur[i, :n] = f["u_right"]
    cnt = np.array([len(f["kps"]) for f in fs], np.int32) if counts is None else np.asarray(counts, np.int32)
    return (kps, desc, ur if batch["stereo"] else None, K, BF if batch["stereo"] else 0.0, BOUNDS, SF, SIGMA2,
            INV_SIGMA2, LOG_SF, cnt)


def last_frame_case(rng, depths, th_depth, held_obs=(), held_noobs=()):
    """an UpdateLastFrame input: depths (n,) as given, random keypoints, descriptors and pose; held_obs /
    held_noobs: slots that hold a MapPoint with / without observations"""
    depths = np.asarray(depths, np.float32)
    n = len(depths)
    kps = np.zeros(n, orbgpu.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    flags = np.zeros(n, np.int32)
    flags[list(held_obs)] = VALID | HAS_OBS
    flags[list(held_noobs)] = VALID
    R = synth._rot(rng, 0.5).astype(np.float32)
    return {"depth": depths, "kps": kps, "desc": rng.integers(0, 256, (n, 32), dtype=np.uint8),
            "K": (K[0], K[1], K[2], K[3], np.float32(1.0) / K[0], np.float32(1.0) / K[1]), "Rwc": R,
            "Ow": rng.uniform(-2, 2, 3).astype(np.float32), "th_depth": np.float32(th_depth), "flags": flags,
            "pos": rng.uniform(-1, 1, (n, 3)).astype(np.float32),
            "mp_desc": rng.integers(0, 256, (n, 32), dtype=np.uint8)}


LAST_SEEN = 8


def chain_local(batch, j, rows, th=3.0, mark_culled=True):
    """Call 2's input as call 1 leaves it, for job j of an initial_batch in motion mode: the local map is the last
    frame's slot table (its points are in the local map), frame_mp is call 1's row after the cull (rows[1]) and
    the points call 1 culled (in rows[0], not in rows[1]) carry LAST_SEEN -- their mnLastFrameSeen is this frame's
    id (Tracking.cpp:1183).  mark_culled=False leaves the flag out: what a caller who forgets it would run.
    Returns a local_batch-shaped dict of one frame and one job; "culled" names (keypoints, points)."""
    J = batch["jobs"][j]
    f, tab = batch["frames"][J["frame"]], J["table"]
    before, after = np.asarray(rows[0], np.int32), np.asarray(rows[1], np.int32)
    kp = np.nonzero((before >= 0) & (after < 0))[0]
    flags = np.array(tab["flags"], np.int32)
    if mark_culled:
        flags[before[kp]] |= LAST_SEEN
    d = tab["pos"].astype(np.float64) - f["C"]
    dist = np.linalg.norm(d, axis=1)
    max_dist = (dist * SF[tab["octave"]] * 0.95).astype(np.float32)
    job = {"frame": 0, "Tcw": None, "frame_mp": after.copy(), "n_local": len(flags), "th": float(th),
           "stereo": int(batch["stereo"]), "only_tracking": 0, "recently_relocalised": 0,
           "table": {"flags": flags, "pos": tab["pos"], "normal": (d / dist[:, None]).astype(np.float32),
                     "desc": tab["desc"], "min_dist": (max_dist / SF[7]).astype(np.float32), "max_dist": max_dist},
           "groups": {"culled": (kp, before[kp])}}
    return _freeze({"stereo": batch["stereo"], "frames": [f], "jobs": [job]})
