"""Constructed scenes for the projection matchers (csrc/proj.hip): the builders of
tests/test_proj_edges.py.

A scene is a dict: name, variant, tgt, pts (the layouts of proj.py / proj_ref.py), th, kw (the
keyword arguments of the search), expect = the oracle's (count, match) and, for the walking
variants, trace = the oracle's trace.  Every scene is deterministic and tiny: identity pose,
fx = fy = 512, cx = 320, cy = 240, points at z = 2 (or -2) over pixel coordinates that are
multiples of 0.25, so every projection is exact in float32.  A builder asserts, with the oracle
only, that its scene reaches the edge it is named after; thresholds that are no multiple of
0.25 px are located by bisecting the oracle's own decision down to two adjacent float32 values.
Families are computed once per process (functools.lru_cache): treat what they return as
read-only."""
from functools import lru_cache

import numpy as np

import proj_ref
from proj_ref import FUSE, FUSE_SIM3, HAS_OBS, IN_VIEW, KEYFRAME, LAST_FRAME, LOCAL, SIM3, SIM3_DIR, VALID

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
FX, CX, CY = 512.0, 320.0, 240.0
WALKERS = (LOCAL, SIM3, LAST_FRAME, KEYFRAME)
PER_POINT = (FUSE, FUSE_SIM3, SIM3_DIR)
ALL = WALKERS + PER_POINT
NAMES = {LOCAL: "local", SIM3: "sim3", LAST_FRAME: "last", KEYFRAME: "kf", FUSE: "fuse", FUSE_SIM3: "fusesim3",
         SIM3_DIR: "sim3dir"}
CLOSED = (LOCAL, LAST_FRAME, KEYFRAME)  # image bounds closed at the far edge (LOCAL: through isInFrustum)
BATCH, CHUNK, LIST_K = 64, 240, 4        # the kernel's walk: lanes per batch, points per chunk, list length


# ---------------------------------------------------------------------------------------------
# inputs

def scale_factors(n_levels):
    return (np.float32(1.2) ** np.arange(n_levels)).astype(np.float32)


def make_target(xy, desc, octave=0, angle=0.0, u_right=None, occupied=None, bounds=(0.0, 640.0, 0.0, 480.0),
                n_levels=8):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    n = len(xy)
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"], k["size"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, -1
    k["octave"], k["angle"] = octave, angle
    return {"kps": k, "desc": np.ascontiguousarray(desc, np.uint8).reshape(n, 32),
            "u_right": None if u_right is None else np.broadcast_to(np.asarray(u_right, np.float32), (n,)).copy(),
            "occupied": None if occupied is None else np.broadcast_to(np.asarray(occupied, np.uint8), (n,)).copy(),
            "min_x": bounds[0], "max_x": bounds[1], "min_y": bounds[2], "max_y": bounds[3],
            "fx": FX, "fy": FX, "cx": CX, "cy": CY, "bf": 40.0, "b": 0.08, "n_levels": n_levels,
            "log_scale_factor": float(np.log(np.float32(1.2))), "scale_factors": scale_factors(n_levels),
            "Tcw": np.eye(4, dtype=np.float32)}


def make_points(uv, desc, z=2.0, flags=VALID | HAS_OBS, octave=None, angle=0.0, level=0, max_dist=None, min_dist=None,
                normal=(0.0, 0.0, 1.0)):
    """points that project exactly onto uv; max_dist defaults to the distance times 1.2^(level - 0.5)
    (the distance itself at level 0), which PredictScale maps to `level`"""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    n = len(uv)
    pos = np.stack([(uv[:, 0] - f32(CX)) * f32(z) / f32(FX), (uv[:, 1] - f32(CY)) * f32(z) / f32(FX),
                    np.full(n, z, np.float32)], 1).astype(np.float32)
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    if max_dist is None:
        max_dist = dist * f32(1.2 ** (level - 0.5)) if level > 0 else dist
    max_dist = np.broadcast_to(np.asarray(max_dist, np.float32), (n,)).copy()
    if min_dist is None:
        min_dist = f32(0.25) * np.minimum(dist, max_dist)
    return {"flags": np.broadcast_to(np.asarray(flags, np.int32), (n,)).copy(), "pos": pos,
            "normal": np.broadcast_to(np.asarray(normal, np.float32), (n, 3)).copy(),
            "desc": np.ascontiguousarray(desc, np.uint8).reshape(n, 32),
            "min_dist": np.broadcast_to(np.asarray(min_dist, np.float32), (n,)).copy(), "max_dist": max_dist,
            "octave": np.broadcast_to(np.asarray(level if octave is None else octave, np.int32), (n,)).copy(),
            "angle": np.broadcast_to(np.asarray(angle, np.float32), (n,)).copy()}


def flip(desc, nbits, start=0):
    """desc with bits start..start+nbits-1 flipped"""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


DEFAULT_TH = {LOCAL: 3.0, SIM3: 10.0, LAST_FRAME: 10.0, KEYFRAME: 10.0, FUSE: 10.0, FUSE_SIM3: 10.0, SIM3_DIR: 10.0}


def default_kw(variant):
    if variant == LOCAL:
        return dict(nnratio=0.9)
    if variant == LAST_FRAME:
        return dict(check_ori=False, mono=True, last_Tcw=np.eye(4, dtype=np.float32))
    if variant == KEYFRAME:
        return dict(check_ori=False, orb_dist=100)
    if variant == SIM3_DIR:
        return dict(last_Tcw=np.eye(4, dtype=np.float32))
    return {}


def run_oracle(sc, trace=None):
    if sc["variant"] in PER_POINT:
        return proj_ref.radius_search(sc["variant"], sc["tgt"], sc["pts"], sc["th"],
                                      last_Tcw=sc["kw"].get("last_Tcw"), trace=trace)
    return proj_ref.search_by_projection(sc["variant"], sc["tgt"], sc["pts"], sc["th"], trace=trace, **sc["kw"])


def scene(name, variant, tgt, pts, th=None, cos_limit=0.5, **kw):
    """the scene with the oracle's result; LOCAL points pass through the oracle's isInFrustum first"""
    if variant == LOCAL:
        fl, tr, lv = proj_ref.is_in_frustum(tgt, pts, cos_limit)
        pts = dict(pts, flags=fl, track=tr, track_level=lv)
    sc = {"name": f"{name}/{NAMES[variant]}", "variant": variant, "tgt": tgt, "pts": pts,
          "th": DEFAULT_TH[variant] if th is None else th, "kw": dict(default_kw(variant), **kw)}
    sc["trace"] = []
    nm, m = run_oracle(sc, sc["trace"])
    m.setflags(write=False)
    sc["expect"] = (nm, m)
    return sc


def hits(sc):
    """number of assignments the oracle made (keypoints for the walkers, points for the others)"""
    return int((sc["expect"][1] >= 0).sum())


# ---------------------------------------------------------------------------------------------
# census of the reference's walk, from the trace alone

def three_maxima(counts):
    """ComputeThreeMaxima on the bin populations: the set of kept bins"""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return {i for i in (i1, i2, i3) if i >= 0}


def census(trace, variant, target, points):
    """What the reference's run implies for a walk that resolves 64 points at a time from lists of
    the 4 best initially visible candidates per point:
      rescans    points with more than 4 initially visible candidates of which fewer than `need`
                 (2 for LOCAL, else 1) of the 4 best are still visible at the point's turn
      conflicts  points with an examined list entry hidden by an earlier point of the same batch
      twice / two_bins / culled / culled_kept  slots assigned more than once / in more than one
                 rotation bin / culled / culled although their last assigner sat in a kept bin
      max_cands  the largest number of candidates passing the non-occupancy filters"""
    need = 2 if variant == LOCAL else 1
    hmin = 2 if variant in (LOCAL, LAST_FRAME) else 1
    occ0 = target.get("occupied")
    occ0 = np.zeros(len(target["kps"]), np.uint8) if occ0 is None else occ0
    batch = lambda ip: (ip // CHUNK, (ip % CHUNK) // BATCH)
    hiders, assigned, bins = {}, {}, {}
    out = {"queries": len(trace), "rescans": 0, "rescan_points": [], "conflicts": 0, "max_cands": 0}
    for rec in trace:
        ip = rec["ip"]
        out["max_cands"] = max(out["max_cands"], len(rec["passed"]))
        vis0 = sorted((d, pos, i) for pos, (i, d, _) in enumerate(rec["passed"]) if occ0[i] < hmin)
        hidden = set(rec["hidden"])
        nvis, examined = 0, []
        for _, _, i in vis0[:LIST_K]:
            if nvis >= need:
                break
            examined.append(i)
            nvis += i not in hidden
        if len(vis0) > LIST_K and nvis < need:
            out["rescans"] += 1
            out["rescan_points"].append(ip)
        if any(h < ip and batch(h) == batch(ip) for i in examined for h in hiders.get(i, ())):
            out["conflicts"] += 1
        s = rec["slot"]
        if s is not None:
            assigned.setdefault(s, []).append((ip, rec["bin"]))
            if (2 if int(points["flags"][ip]) & HAS_OBS else 1) >= hmin:
                hiders.setdefault(s, []).append(ip)
            if rec["bin"] is not None:
                bins.setdefault(s, set()).add(rec["bin"])
    counts = [0] * proj_ref.HL
    for a in assigned.values():
        for _, b in a:
            if b is not None:
                counts[b] += 1
    keep = three_maxima(counts)
    out["twice"] = sum(len(a) > 1 for a in assigned.values())
    out["two_bins"] = sum(len(b) > 1 for b in bins.values())
    out["culled"] = sum(bool(b - keep) for b in bins.values())
    out["culled_kept"] = sum(bool(bins[s] - keep) and a[-1][1] in keep for s, a in assigned.items() if s in bins)
    return out


def scene_census(sc):
    return census(sc["trace"], sc["variant"], sc["tgt"], sc["pts"])


# ---------------------------------------------------------------------------------------------
# the stacked scene

GROUPS, COLS, PER_GROUP = 54, 9, 8
OFFSETS = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1)]
ROT_BINS = [0, 0, 0, 5, 5, 10, 10, 0]  # rotation bin of a group's p-th point (keypoint angles are 0)


def stacked(variant, groups=GROUPS, ppg=PER_GROUP, kpg=8, has_obs=True, check_ori=False, nnratio=0.9, interleave=False,
            drop=0, keep=None, filler=0, z=2.0, name="stacked", **search_kw):
    """`groups` clusters on a 64 px lattice, each `kpg` (8) octave-0 keypoints within 1 px of the centre,
    keypoint j carrying the group's descriptor with its first 3j bits flipped, and `ppg` points
    with the group's descriptor projecting onto the centre, in group order: the first point takes
    keypoint 0, the next keypoint 1 ... -- or, where an assignment does not hide (LAST_FRAME and
    LOCAL points without observations), all of them keypoint 0.  `filler` keypoints outside every
    window come first, so the clusters hold the highest slots; the clusters' own slots are
    shuffled.  Points: the first `drop` removed, then cut to `keep`.  With check_ori the points'
    angles put a group's assignments into bins 0, 5 and 10, point 1 of every fifth group into
    bin 15 and point 6 of every fifth group into bin 20 (both culled)."""
    rng = np.random.default_rng(5)
    gdesc = rng.integers(0, 256, (GROUPS, 32), dtype=np.uint8)[:groups]
    centres = np.array([(64.0 + 64.0 * (g % COLS), 64.0 + 64.0 * (g // COLS)) for g in range(groups)], np.float32)
    nk = 1 if filler < 0 else kpg  # filler = -1: a one-keypoint target
    kxy = np.array([centres[g] + np.array(OFFSETS[j], np.float32) for g in range(groups) for j in range(nk)])
    kdesc = np.array([flip(gdesc[g], 3 * j) for g in range(groups) for j in range(nk)])
    perm = rng.permutation(len(kxy))
    kxy, kdesc = kxy[perm], kdesc[perm]
    if filler > 0:  # a band below the clusters, 0.25 px apart in x, far from every window
        fi = np.arange(filler)
        fxy = np.stack([(fi % 2048) * 0.25 + 64.0, 440.0 + 8.0 * (fi // 2048)], 1).astype(np.float32)
        kxy = np.concatenate([fxy, kxy])
        kdesc = np.concatenate([rng.integers(0, 256, (filler, 32), dtype=np.uint8), kdesc])
    tgt = make_target(kxy, kdesc)
    order = [(g, p) for g in range(groups) for p in range(ppg)]
    if interleave:
        order = [(g, p) for p in range(ppg) for g in range(groups)]
    order = order[drop:][:keep]
    bins = []
    for g, p in order:
        b = ROT_BINS[p % 8]
        if g % 5 == 2 and p == 1:
            b = 15
        if g % 5 == 3 and p == 6:
            b = 20
        bins.append(b)
    pts = make_points([centres[g] for g, _ in order], [gdesc[g] for g, _ in order], z=z,
                      flags=VALID | (HAS_OBS if has_obs else 0), angle=12.0 * np.array(bins, np.float32))
    kw = dict(search_kw)
    if variant == LOCAL:
        kw["nnratio"] = nnratio
    if variant in (LAST_FRAME, KEYFRAME):
        kw["check_ori"] = check_ori
    return scene(name, variant, tgt, pts, **kw)


@lru_cache(maxsize=None)
def stacked_family():
    """name -> scene; the walking variants over the stacked scene and its variations"""
    out = {}

    def add(sc, **req):
        c = scene_census(sc)
        first = sum(ip < CHUNK for ip in c["rescan_points"])
        for key, lo in req.items():
            have = first if key == "rescans_first_chunk" else c[key.replace("_below", "")]
            assert (have < lo) if key.endswith("_below") else (have >= lo), (sc["name"], key, have, lo, c)
        sc["census"] = c
        out[sc["name"]] = sc
        return c

    for v in WALKERS:
        add(stacked(v), rescans_first_chunk=100, conflicts=200)
        # dropping 5 points puts a rescanned point on a batch's lane 0 (point 64), on lane 63 and on
        # point 240, the first of the second chunk
        c = add(stacked(v, drop=5, name="stacked-drop5"), rescans_first_chunk=100, conflicts=200)
        assert {63, 64, 240} <= set(c["rescan_points"]), c["rescan_points"]
        add(stacked(v, interleave=True, name="stacked-interleaved"), conflicts_below=50, rescans=100)
        for keep in (63, 64, 65, 239, 240, 241, 481):  # 9 points a group: a group straddles every boundary
            sc = stacked(v, ppg=9, drop=3, keep=keep, name=f"stacked-cut{keep}")
            assert len(sc["pts"]["flags"]) == keep
            add(sc, rescans=20)
        # 5 keypoints a group: the shortest list that is truncated; 4: the longest that is not, and runs out
        c = add(stacked(v, groups=16, kpg=5, name="stacked-five"), rescans=16, conflicts=100)
        assert c["max_cands"] == 5
        c = add(stacked(v, groups=16, kpg=4, name="stacked-four"), conflicts=100)
        assert c["max_cands"] == 4 and c["rescans"] == 0
    # assignments that do not hide: every point of a group takes keypoint 0
    for v in (LAST_FRAME, LOCAL):
        c = add(stacked(v, has_obs=False, name="stacked-noobs"), twice=40)
        assert c["rescans"] == 0
    c = add(stacked(LAST_FRAME, has_obs=False, check_ori=True, name="stacked-noobs-ori"), twice=40, two_bins=5,
            culled_kept=1)
    # a stereo frame that moved forward / backward along z by more than the baseline: the level window
    # becomes "the point's octave and up" / "0 .. the point's octave"
    for tag, tz in (("forward", 1.0), ("backward", -1.0)):
        last = np.eye(4, dtype=np.float32)
        last[2, 3] = tz
        add(stacked(LAST_FRAME, groups=16, mono=False, last_Tcw=last, name=f"stacked-{tag}"), rescans=60,
            conflicts=100)
    for v in (LAST_FRAME, KEYFRAME):  # one assignment a slot; rescanned points land in kept and culled bins
        sc = stacked(v, check_ori=True, name="stacked-ori")
        c = add(sc, rescans_first_chunk=100, culled=10)
        assert (sc["expect"][1] == -2).sum() == c["culled"] >= 20
    # nnratio 0.8: 12 against 0.8 * 15 sits on the equality (accepted), 15 against 0.8 * 18 is rejected, so
    # the points after it see the same best again
    sc = stacked(LOCAL, nnratio=0.8, name="stacked-nn0.8")
    add(sc, rescans_first_chunk=100, conflicts=200)
    by_ip = {r["ip"]: r for r in sc["trace"]}
    best = lambda r: min((d, i) for i, d, _ in r["passed"] if i not in r["hidden"])
    assert by_ip[4]["slot"] is not None and best(by_ip[4])[0] == 12
    assert by_ip[5]["slot"] is None and by_ip[6]["slot"] is None and best(by_ip[5]) == best(by_ip[6])
    assert best(by_ip[5])[0] == 15
    return out


# ---------------------------------------------------------------------------------------------
# one keypoint, one point

def single(variant, name, u=320.0, v=240.0, kx=None, ky=None, level=0, koct=None, hamming=0, **o):
    """one point projecting onto (u, v) and one keypoint at (kx, ky) (default: the same place) with
    the point's descriptor but `hamming` flipped bits.  Options: bounds, n_levels, u_right,
    occupied, z, normal, max_dist, min_dist, flags, th, cos_limit, and the search's keywords."""
    d = np.random.default_rng(11).integers(0, 256, 32, dtype=np.uint8)
    tk = {k: o.pop(k) for k in ("bounds", "n_levels", "u_right", "occupied") if k in o}
    pk = {k: o.pop(k) for k in ("z", "normal", "max_dist", "min_dist", "flags") if k in o}
    tgt = make_target([(u if kx is None else kx, v if ky is None else ky)], [d],
                      octave=level if koct is None else koct, **tk)
    pts = make_points([(u, v)], [flip(d, hamming)], level=level, **pk)
    return scene(name, variant, tgt, pts, **o)


def _ord(x):
    """float32 -> an integer that orders like the float"""
    i = int(np.float32(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _unord(i):
    return np.int32(i).view(np.float32) if i >= 0 else np.int32((-i) | -0x80000000).view(np.float32)


def straddle(build, a, b):
    """the two adjacent float32 values between a and b at which the oracle's verdict on build(value)
    changes: build returns a scene, the verdict is whether it assigns anything.  Returns both
    scenes, the matching one first."""
    sa, sb = build(f32(a)), build(f32(b))
    assert hits(sa) != hits(sb), (sa["name"], a, b)
    ia, ib = _ord(a), _ord(b)
    while abs(ia - ib) > 1:
        im = (ia + ib) // 2
        sm = build(_unord(im))
        if hits(sm) == hits(sa):
            ia, sa = im, sm
        else:
            ib, sb = im, sm
    sa["value"], sb["value"] = _unord(ia), _unord(ib)
    return (sa, sb) if hits(sa) else (sb, sa)


def _put(out, *scs):
    for sc in scs:
        assert sc["name"] not in out, sc["name"]
        out[sc["name"]] = sc


EDGE_BOUNDS = (16.0, 600.0, 8.0, 440.0)
GRID_BOUNDS = (-12.5, 655.25, -7.75, 489.0)


@lru_cache(maxsize=None)
def bounds_family():
    """image bounds: a point a quarter pixel inside, on and a quarter pixel outside each of the four
    edges, level 7 with the keypoint 5 px inside the edge (the grid drops keypoints in its last half
    cell, and Fuse's chi-square needs 5 px to be small against the level's sigma)"""
    out = {}
    for v in ALL:
        for edge, val in zip(("minx", "maxx", "miny", "maxy"), EDGE_BOUNDS):
            far = edge.startswith("max")
            for side, off in (("in", -0.25 if far else 0.25), ("on", 0.0), ("out", 0.25 if far else -0.25)):
                p = val + off
                kp = val + (-5.0 if far else 5.0)
                at = dict(u=p, kx=kp) if edge.endswith("x") else dict(v=p, ky=kp)
                sc = single(v, f"bounds-{edge}-{side}", level=7, bounds=EDGE_BOUNDS, **at)
                want = side == "in" or (side == "on" and (not far or v in CLOSED))
                assert hits(sc) == int(want), (sc["name"], sc["expect"])
                _put(out, sc)
    # a level-0 window in the middle of an image whose bounds do not start at 0: the keypoint a quarter
    # pixel inside each of the window's four edges
    for v in ALL:
        r = {LOCAL: 7.5, FUSE: 2.0}.get(v, 10.0)
        for btag, bounds in (("edge", EDGE_BOUNDS), ("grid", GRID_BOUNDS)):
            for tag, dx, dy in (("x+", r - 0.25, 0.0), ("x-", 0.25 - r, 0.0), ("y+", 0.0, r - 0.25),
                                ("y-", 0.0, 0.25 - r)):
                sc = single(v, f"offset-{btag}-{tag}", kx=320.0 + dx, ky=240.0 + dy, bounds=bounds,
                            th=_window_th(v))
                assert hits(sc) == 1, (sc["name"], sc["expect"])
                _put(out, sc)
    return out


def _window_th(v):
    return 2.0 if v == FUSE else None  # keeps the window's edge inside Fuse's chi-square gate


@lru_cache(maxsize=None)
def window_family():
    """the strict window test |dx| < r, |dy| < r at levels 0 and 3, on both sides of the point"""
    out = {}
    for v in ALL:
        for level in (0, 3):
            for axis in "xy":
                for sign in (1.0, -1.0):
                    def build(val, v=v, level=level, axis=axis):
                        at = dict(kx=val) if axis == "x" else dict(ky=val)
                        return single(v, f"window-{axis}{'+' if sign > 0 else '-'}-l{level}", level=level,
                                      th=_window_th(v), **at)
                    c = 320.0 if axis == "x" else 240.0
                    a, b = straddle(build, c + sign * 0.25, c + sign * 60.0)
                    if level == 0:  # r is a whole number of half pixels: the keypoint exactly r away is outside
                        r = abs(float(b["value"]) - c)
                        assert 2 * r == int(2 * r) and abs(float(a["value"]) - c) < r, (b["name"], r)
                    a["name"] += "-in"
                    b["name"] += "-out"
                    _put(out, a, b)
    return out


@lru_cache(maxsize=None)
def stereo_family():
    """the stereo gate er > r (LOCAL, LAST_FRAME), u_right of 0, -1 and a small positive value in the
    searches and in Fuse, and Fuse's chi-square limits 5.99 / 7.8 at octaves 0 and 3"""
    out = {}
    for v in (LOCAL, LAST_FRAME):
        for sign in (1.0, -1.0):  # the projected right coordinate is 320 - 40 / 2 = 300
            build = lambda val, v=v: single(v, f"stereo-gate{'+' if sign > 0 else '-'}", u_right=val)
            a, b = straddle(build, 300.0 + sign * 0.25, 300.0 + sign * 100.0)
            r = abs(float(a["value"]) - 300.0)
            assert 2 * r == int(2 * r), (a["name"], r)  # er == r passes (r = 10, or 7.5 for LOCAL)
            a["name"] += "-in"
            b["name"] += "-out"
            _put(out, a, b)
    for v in ALL:
        want = {"zero": v != FUSE, "minus1": True, "tiny": v not in (LOCAL, LAST_FRAME, FUSE)}
        for tag, ur in (("zero", 0.0), ("minus1", -1.0), ("tiny", 2.0 ** -10)):
            sc = single(v, f"uright-{tag}", u_right=ur)
            assert hits(sc) == int(want[tag]), (sc["name"], sc["expect"])
            _put(out, sc)
    for level in (0, 3):
        for tag, ur in (("mono", -1.0), ("stereo", 300.0), ("stereo-off", 301.0)):
            build = lambda val: single(FUSE, f"chi2-{tag}-l{level}", level=level, u_right=ur, kx=val, ky=240.75,
                                       th=4.0)
            a, b = straddle(build, 320.0, 330.0)
            a["name"] += "-in"
            b["name"] += "-out"
            _put(out, a, b)
    return out


@lru_cache(maxsize=None)
def distance_family():
    """the distance against 0.8 min_dist and 1.2 max_dist, the viewing angle against 0.5 (and against
    isInFrustum's limit for LOCAL), PredictScale's clamps and level steps"""
    out = {}

    def pair(a, b):
        a["name"] += "-in"
        b["name"] += "-out"
        _put(out, a, b)

    for v in (LOCAL, SIM3, KEYFRAME, FUSE, FUSE_SIM3, SIM3_DIR):  # the point sits 2 away
        pair(*straddle(lambda val, v=v: single(v, "dist-min", min_dist=val), 1.0, 4.0))
        pair(*straddle(lambda val, v=v: single(v, "dist-max", max_dist=val, min_dist=0.5), 2.0, 1.0))
    for v in (SIM3, FUSE, FUSE_SIM3):
        a, b = straddle(lambda val, v=v: single(v, "view-angle", normal=(0.0, 0.0, val)), 1.0, 0.125)
        assert float(a["value"]) == 0.5
        pair(a, b)
    for lim in (0.5, 0.8):
        pair(*straddle(lambda val: single(LOCAL, f"view-limit{lim}", normal=(0.0, 0.0, val), cos_limit=lim),
                       1.0, 0.125))
    for v in (LOCAL, SIM3, KEYFRAME, FUSE, FUSE_SIM3, SIM3_DIR):
        top = 1 if v == KEYFRAME else 0  # the keypoint level just inside the window's upper end
        for k in (0, 2, 6):  # max_dist / dist either side of 1.2^k: level k against k + 1
            build = lambda val, v=v, k=k: single(v, f"scale-step{k}", max_dist=val, min_dist=0.5,
                                                 koct=k + 1 + top, th=3.0 if v == FUSE else None)
            pair(*straddle(build, 2.0 * 1.2 ** (k + 0.5), 2.0 * 1.2 ** (k - 0.5)))
        # a ratio below 1 gives level 0 (never -1), a huge one the last level (never one past it)
        for tag, kw in (("ratio-low", dict(max_dist=1.75, koct=0)),
                        ("ratio-huge", dict(max_dist=2.0e6, koct=6)),
                        ("levels1", dict(max_dist=2.0e6, koct=0, n_levels=1)),
                        ("levels16", dict(max_dist=2.0e6, koct=14, n_levels=16))):
            sc = single(v, f"scale-{tag}", min_dist=0.5, **kw)
            assert hits(sc) == 1, (sc["name"], sc["expect"])
            _put(out, sc)
    return out


@lru_cache(maxsize=None)
def hamming_family():
    """the distance thresholds 50, 100 and orb_dist, the ratio test's equality, occupancy"""
    out = {}
    for v in ALL:
        limits = {KEYFRAME: (0, 64, 255)}.get(v, (50,) if v in (SIM3, FUSE, FUSE_SIM3) else (100,))
        for lim in limits:
            kw = dict(orb_dist=lim) if v == KEYFRAME else {}
            a = single(v, f"hamming-{lim}", hamming=lim, **kw)
            b = single(v, f"hamming-{lim + 1}", hamming=lim + 1, **kw)
            assert (hits(a), hits(b)) == (1, 0), (a["name"], a["expect"], b["expect"])
            _put(out, a, b)
    d = np.random.default_rng(12).integers(0, 256, 32, dtype=np.uint8)

    def two(name, best, second, octs, nnratio, want, level=1):
        tgt = make_target([(320.0, 240.0), (321.0, 240.0)], [flip(d, best), flip(d, second, 100)], octave=octs)
        sc = scene(name, LOCAL, tgt, make_points([(320.0, 240.0)], [d], level=level), nnratio=nnratio)
        assert hits(sc) == int(want), (name, sc["expect"])
        _put(out, sc)

    two("ratio-on", 12, 15, (1, 1), 0.8, True)        # 12 > 0.8f * 15 is false: the product rounds to 12
    two("ratio-over", 13, 15, (1, 1), 0.8, False)
    two("ratio-levels-differ", 13, 15, (1, 0), 0.8, True)
    two("ratio-second-first", 15, 13, (0, 1), 0.8, True)  # the better one comes second in the window
    two("ratio-equal-dists", 13, 13, (1, 1), 0.99, False)
    sc = single(LOCAL, "ratio-lone", hamming=100, nnratio=0.01)
    assert hits(sc) == 1
    _put(out, sc)
    for v in ALL:
        for occ in (0, 1, 2):
            sc = single(v, f"occupied-{occ}", occupied=occ)
            hidden = v in WALKERS and occ >= (2 if v in (LOCAL, LAST_FRAME) else 1)
            assert hits(sc) == int(not hidden), (sc["name"], sc["expect"])
            _put(out, sc)
    return out


@lru_cache(maxsize=None)
def depth_family():
    """z = -2: only KEYFRAME has no depth test, and its mirrored projection lands on the clusters"""
    out = {}
    for v in ALL:
        sc = stacked(v, groups=6, z=-2.0, name="negative-depth")
        assert (hits(sc) > 0) == (v == KEYFRAME), (sc["name"], sc["expect"][0])
        if v == KEYFRAME:
            assert sc["expect"][0] == 48
        _put(out, sc)
    return out


@lru_cache(maxsize=None)
def ties_family():
    """two keypoints at the same Hamming distance: the first in GetFeaturesInArea order wins (columns
    outer, rows inner, slot order within a cell)"""
    out = {}
    d = np.random.default_rng(13).integers(0, 256, 32, dtype=np.uint8)
    places = {"one-cell": [(320.0, 240.0), (320.5, 240.5)],
              "two-rows": [(320.0, 245.25), (320.5, 244.75)],       # rows 25 and 24 of column 32
              "two-columns": [(325.25, 240.0), (324.75, 240.5)]}    # columns 33 and 32: slot 1 comes first
    for v in ALL:
        for tag, kxy in places.items():
            for dist in (0, 7):
                # levels 1 and 0 under a level-1 point: LOCAL's ratio test then lets the tie through
                tgt = make_target(kxy, [flip(d, dist), flip(d, dist, 128)], octave=(1, 0))
                uv = np.mean(kxy, 0)
                sc = scene(f"tie-{tag}-d{dist}", v, tgt, make_points([uv], [d], level=1))
                grid = proj_ref.Grid(tgt)
                cells = [(ix, iy) for ix in range(64) for iy in range(48) for _ in grid.cells[ix][iy]]
                assert len(set(cells)) == (1 if tag == "one-cell" else 2), cells
                (rec,) = sc["trace"]
                assert [p[1] for p in rec["passed"]] == [dist, dist], rec
                assert rec["slot"] == rec["cands"][0] == (0 if tag == "one-cell" else 1), rec
                _put(out, sc)
    return out


@lru_cache(maxsize=None)
def grid_family():
    """bounds that are no whole numbers: keypoints that round into the last cell of each axis and into
    cell 0, their neighbours a quarter pixel on that round outside the grid, and windows clamped at
    both ends of both axes"""
    out = {}
    rng = np.random.default_rng(14)
    # (keypoint, inside the grid?, the point looking at it)
    spots = [((649.75, 200.0), True, (648.0, 200.0)), ((650.25, 260.0), False, (648.0, 260.0)),
             ((200.0, 483.75), True, (200.0, 482.0)), ((260.0, 484.0), False, (260.0, 482.0)),
             ((-17.5, 100.0), True, (-12.25, 100.0)), ((-18.0, 160.0), False, (-12.25, 160.0)),
             ((100.0, -12.75), True, (100.0, -7.5)), ((160.0, -13.0), False, (160.0, -7.5)),
             ((649.75, 483.75), True, (655.0, 488.75)), ((-17.5, -12.75), True, (-12.5, -7.75)),
             ((320.0, 240.0), True, (320.0, 240.0))]
    kxy = [s[0] for s in spots]
    desc = rng.integers(0, 256, (len(spots), 32), dtype=np.uint8)
    for v in ALL:
        tgt = make_target(kxy, desc, octave=7, bounds=GRID_BOUNDS)
        grid = proj_ref.Grid(tgt)
        where = {i: (ix, iy) for ix in range(64) for iy in range(48) for i in grid.cells[ix][iy]}
        assert set(where) == {i for i, s in enumerate(spots) if s[1]}, where
        assert where[0][0] == 63 and where[2][1] == 47 and where[8] == (63, 47) and where[9] == (0, 0), where
        sc = scene("grid-edges", v, tgt, make_points([s[2] for s in spots], desc, level=7))
        nm, m = sc["expect"]
        got = set(np.nonzero(m >= 0)[0]) if v in WALKERS else set(m[m >= 0])
        assert got <= set(where) and (v == FUSE or got == set(where)), (sc["name"], got)
        _put(out, sc)
    return out


def rotation_scene(variant, name, groups, check_ori=True):
    """groups = [(count, angle difference)]: that many lone keypoint / point pairs with the point's
    angle minus the keypoint's equal to the difference; the last two keypoints have no point"""
    diffs = [d for c, d in groups for _ in range(c)]
    n = len(diffs)
    rng = np.random.default_rng(15)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    xy = np.array([(32.0 + 32.0 * (i % 18), 32.0 + 32.0 * (i // 18)) for i in range(n)], np.float32)
    kang = np.where(np.array(diffs) < 0, 30.0, 0.25).astype(np.float32)
    lone = np.array([(32.0, 400.0), (96.0, 400.0)], np.float32)
    tgt = make_target(np.concatenate([xy, lone]), np.concatenate([desc, 255 - desc[:2]]),
                      angle=np.concatenate([kang, [7.0, 8.0]]))
    pts = make_points(xy, desc, angle=(kang.astype(np.float64) + np.array(diffs)).astype(np.float32))
    sc = scene(name, variant, tgt, pts, check_ori=check_ori)
    assert (sc["expect"][1][n:] == -1).all()
    return sc


@lru_cache(maxsize=None)
def rotation_family():
    out = {}
    for v in (LAST_FRAME, KEYFRAME):
        def add(name, groups, kept, check_ori=True):
            """kept: per group, whether its matches survive the cull"""
            sc = rotation_scene(v, name, groups, check_ori)
            m, i = sc["expect"][1], 0
            for (c, _), k in zip(groups, kept):
                assert (m[i:i + c] >= 0).all() if k else (m[i:i + c] == -2).all(), (sc["name"], m)
                i += c
            assert sc["expect"][0] == sum(c for (c, _), k in zip(groups, kept) if k)
            _put(out, sc)
            return sc
        # 353.9 -> bin 29, 354.1 -> bin 30 = bin 0, 6.0 -> 0.5 rounds away from zero to bin 1, -20 -> 340
        sc = add("rot-bins", [(3, 353.875), (4, 354.125), (5, 6.0), (2, -20.0)], [True, True, True, False])
        assert [r["bin"] for r in sc["trace"]] == [29] * 3 + [0] * 4 + [1] * 5 + [28] * 2
        sc = add("rot-wrap-joins-zero", [(2, 354.125), (2, 1.0), (3, 100.0), (3, 200.0), (1, 300.0)],
                 [True, True, True, True, False])
        assert [r["bin"] for r in sc["trace"]][:4] == [0] * 4
        add("rot-second-10-1", [(10, 0.0), (1, 100.0)], [True, True])
        add("rot-second-11-1", [(11, 0.0), (1, 100.0)], [True, False])
        add("rot-third-10-5-1", [(10, 0.0), (5, 100.0), (1, 200.0), (1, 300.0)], [True, True, True, False])
        add("rot-third-11-5-1", [(11, 0.0), (5, 100.0), (1, 200.0)], [True, True, False])
        add("rot-tied", [(3, 300.0), (3, 200.0), (3, 100.0), (3, 0.0)], [False, True, True, True])
        add("rot-tied-second", [(5, 300.0), (3, 200.0), (3, 100.0), (3, 0.0)], [True, False, True, True])
        add("rot-one-bin", [(5, 123.0)], [True])
        add("rot-off", [(11, 0.0), (1, 100.0)], [True, True], check_ori=False)
    return out


@lru_cache(maxsize=None)
def capacity_family():
    """targets of 1, 2047, 2048 (the last with descriptors on chip), 2049, 4095 and 4096 keypoints: four
    clusters in the highest slots, the rest filler outside every window"""
    out = {}
    for v in ALL:
        for n in (1, 2047, 2048, 2049, 4095, 4096):
            sc = stacked(v, groups=1 if n == 1 else 4, filler=-1 if n == 1 else n - 32, name=f"capacity-{n}")
            assert len(sc["tgt"]["kps"]) == n
            m = sc["expect"][1]
            if v in WALKERS and n > 1:
                assert (m[:n - 32] == -1).all() and (m[n - 32:] >= 0).all(), sc["name"]
            else:
                assert hits(sc) > 0, sc["name"]
            _put(out, sc)
    return out


FAMILIES = {"stacked": stacked_family, "bounds": bounds_family, "window": window_family, "stereo": stereo_family,
            "distance": distance_family, "hamming": hamming_family, "depth": depth_family, "ties": ties_family,
            "grid": grid_family, "rotation": rotation_family, "capacity": capacity_family}


# ---------------------------------------------------------------------------------------------
# isInFrustum

@lru_cache(maxsize=None)
def frustum_case():
    """(tgt, pts, cos_limit, (flags, track, level) of the oracle): 257 points, the straddle pairs of the
    bounds (closed on all four sides), the distance limits, the viewing angle and the level steps, tiled;
    every point enters with IN_VIEW set"""
    tgt = make_target([(320.0, 240.0)], np.zeros((1, 32), np.uint8), bounds=EDGE_BOUNDS)
    rows = []  # (u, v, min_dist, max_dist, nz)

    def verdict(row):
        u, v, mn, mx, nz = row
        p = make_points([(u, v)], np.zeros((1, 32), np.uint8), min_dist=mn, max_dist=mx, normal=(0.0, 0.0, nz))
        fl, _, lv = proj_ref.is_in_frustum(tgt, p, 0.5)
        return (int(fl[0]) & IN_VIEW, int(lv[0]))

    def bisect(make, a, b):
        ia, ib = _ord(a), _ord(b)
        va = verdict(make(_unord(ia)))
        assert va != verdict(make(_unord(ib))), (a, b)
        while abs(ia - ib) > 1:
            im = (ia + ib) // 2
            if verdict(make(_unord(im))) == va:
                ia = im
            else:
                ib = im
        rows.extend([make(_unord(ia)), make(_unord(ib))])

    x0, x1, y0, y1 = EDGE_BOUNDS
    for u, v, inside in [(x0, 240.0, 1), (x0 - 0.25, 240.0, 0), (x1, 240.0, 1), (x1 + 0.25, 240.0, 0),
                         (320.0, y0, 1), (320.0, y0 - 0.25, 0), (320.0, y1, 1), (320.0, y1 + 0.25, 0)]:
        d = float(np.sqrt(((u - CX) / 256.0) ** 2 + ((v - CY) / 256.0) ** 2 + 4.0))
        rows.append((u, v, 0.5 * d, d, 1.0))
        assert bool(verdict(rows[-1])[0]) == bool(inside), rows[-1]
    bisect(lambda val: (320.0, 240.0, val, 2.0, 1.0), 1.0, 4.0)        # dist against 0.8 min_dist
    bisect(lambda val: (320.0, 240.0, 0.5, val, 1.0), 2.0, 1.0)        # dist against 1.2 max_dist
    bisect(lambda val: (320.0, 240.0, 0.5, 2.0, val), 1.0, 0.125)      # viewing cosine against 0.5
    for k in range(0, 8):                                              # level k against k + 1 (7 is the last)
        if k < 7:
            bisect(lambda val: (320.0, 240.0, 0.5, val, 1.0), 2.0 * 1.2 ** (k + 0.5), 2.0 * 1.2 ** (k - 0.5))
    rows.append((320.0, 240.0, 0.5, 2.0e6, 1.0))   # clamped to the last level
    rows.append((320.0, 240.0, 0.5, 1.75, 1.0))    # a ratio below 1: level 0
    rows.append((320.0, 240.0, 0.5, 2.0, -1.0))    # seen from behind
    rows = [rows[i % len(rows)] for i in range(257)]
    r = np.array(rows, np.float64)
    pts = make_points(r[:, :2], np.zeros((257, 32), np.uint8), min_dist=r[:, 2], max_dist=r[:, 3],
                      flags=VALID | HAS_OBS | IN_VIEW)
    pts["normal"][:, 2] = r[:, 4]
    exp = proj_ref.is_in_frustum(tgt, pts, 0.5)
    inv = (exp[0] & IN_VIEW) != 0
    assert 20 < inv.sum() < 237 and set(exp[2][inv]) == set(range(8)), (inv.sum(), set(exp[2][inv]))
    return tgt, pts, 0.5, exp
