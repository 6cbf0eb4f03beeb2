"""Small constructed maps for Tracking::UpdateLocalMap (csrc/localmap.hip,
tests/localmap_ref.py), in the manner of track_scene.py: a scene is built from
named groups of keyframes and points, and the names come back so a test can
assert on what each group is there to show.

``Map`` builds a mirror (include/orbgpu_localmap.h) and one frame's job by hand:

  kf(n, bad=False)        n keyframes; returns their indices
  point(kfs, bad, obs)    a map point in a fresh slot of every keyframe of `kfs`,
                          observed from them (obs=False: the slots hold it, the
                          point lists no observation and has no HAS_OBS)
  null(kf, n)             n NULL slots
  covis / child / parent  the covisibility list (longer than 10: the mirror gets
                          the first 10), a child, the parent
  hold(p, times=1)        keypoints whose mvpMapPoints is p after call 1 (rows 0
                          and 1); times=2: one table entry at two keypoints
  cull(p)                 a keypoint call 1 matched to p and culled (row 0 only)
  vo()                    a temporal visual-odometry point (src_pt_id -1), held
  free(n)                 keypoints that hold nothing

Descriptors, positions, normals and distances are random: the call copies them.
``SCENES`` names the constructed cases; ``sized`` makes the edge sizes.
"""
from __future__ import annotations

import numpy as np

VALID, HAS_OBS = 1, 2


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


class Map:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.bad, self.slots, self.cov, self.children, self.par = [], [], [], [], []
        self.pt_flags, self.obs = [], []
        self.src, self.row0, self.row1 = [], [], []
        self.entry = {}
        self.rank, self.prev = None, []

    # ---- the map
    def kf(self, n=1, bad=False):
        first = len(self.bad)
        for _ in range(n):
            self.bad.append(int(bad))
            self.slots.append([])
            self.cov.append([])
            self.children.append([])
            self.par.append(-1)
        return list(range(first, first + n))

    def point(self, kfs=(), bad=False, obs=True):
        p = len(self.pt_flags)
        self.pt_flags.append((0 if bad else VALID) | (HAS_OBS if obs and len(kfs) else 0))
        self.obs.append(list(kfs) if obs else [])
        for k in kfs:
            self.slots[k].append(p)
        return p

    def points(self, n, kfs=(), **kw):
        return [self.point(kfs, **kw) for _ in range(n)]

    def put(self, kf, p):
        """p in a further slot of kf, without an observation of its own"""
        self.slots[kf].append(p)

    def null(self, kf, n=1):
        self.slots[kf] += [-1] * n

    def covis(self, kf, others):
        self.cov[kf] = list(others)

    def child(self, kf, c):
        self.children[kf].append(c)

    def parent(self, kf, p):
        self.par[kf] = p

    # ---- the frame after call 1
    def _entry(self, p):
        if p not in self.entry:
            self.entry[p] = len(self.src)
            self.src.append(p)
        return self.entry[p]

    def hold(self, p, times=1):
        t = self._entry(p)
        kp = list(range(len(self.row0), len(self.row0) + times))
        self.row0 += [t] * times
        self.row1 += [t] * times
        return kp

    def cull(self, p):
        self.row0.append(self._entry(p))
        self.row1.append(-1)
        return len(self.row0) - 1

    def vo(self, times=1):
        t = len(self.src)
        self.src.append(-1)
        kp = list(range(len(self.row0), len(self.row0) + times))
        self.row0 += [t] * times
        self.row1 += [t] * times
        return t, kp

    def free(self, n=1):
        self.row0 += [-1] * n
        self.row1 += [-1] * n

    def unused_entries(self, n):
        """entries of call 1's table that no keypoint matched"""
        for _ in range(n):
            self.src.append(int(self.rng.integers(-1, max(len(self.pt_flags), 1))) if self.pt_flags else -1)

    def done(self, **names):
        rng = self.rng
        n_kf, n_pt, n_src = len(self.bad), len(self.pt_flags), len(self.src)
        covis = np.full((n_kf, 10), -1, np.int32)
        for k, c in enumerate(self.cov):
            covis[k, :min(len(c), 10)] = c[:10]
        d = rng.uniform(1.0, 8.0, n_pt).astype(np.float32)
        normal = rng.normal(size=(n_pt, 3))
        normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-9)
        mirror = {"kf_bad": np.array(self.bad, np.uint8), "slots": [np.array(s, np.int32) for s in self.slots],
                  "covis": covis, "children": [list(c) for c in self.children], "parent": np.array(self.par, np.int32),
                  "kf_by_rank": None if self.rank is None else np.array(self.rank, np.int32),
                  "pt_flags": np.array(self.pt_flags, np.int32), "obs": [list(o) for o in self.obs],
                  "pos": rng.uniform(-5, 5, (n_pt, 3)).astype(np.float32), "normal": normal.astype(np.float32),
                  "desc": rng.integers(0, 256, (n_pt, 32), dtype=np.uint8), "min_dist": (d * np.float32(0.3)),
                  "max_dist": d}
        job = {"n_kp": len(self.row0), "rows": np.array([self.row0, self.row1], np.int32).reshape(2, -1),
               "src_pt_id": np.array(self.src, np.int32), "src_pos": rng.uniform(-5, 5, (n_src, 3)).astype(np.float32),
               "src_desc": rng.integers(0, 256, (n_src, 32), dtype=np.uint8), "prev_kfs": list(self.prev)}
        return _freeze({"mirror": mirror, "job": job, "names": names})


# ---- the K2 walk ---------------------------------------------------------------

def k1_of(n):
    """K1 of n members, each with one vote and one covisible outside K1 that nothing else names"""
    m = Map(100 + n)
    k1 = m.kf(n)
    extra = m.kf(n)
    for a, b in zip(k1, extra):
        m.hold(m.point([a]))
        m.covis(a, [b])
        m.points(2, [b])
    return m.done(k1=k1, extra=extra)


def parent_break():
    m = Map(201)
    a, b, c = m.kf(3)
    par, na, nb, nc = m.kf(4)
    for k in (a, b, c):
        m.hold(m.point([k]))
    m.covis(a, [na])
    m.covis(b, [nb])
    m.covis(c, [nc])
    m.parent(a, par)  # unmarked: appended, and the walk ends before b and c are visited
    return m.done(k1=[a, b, c], parent=par, first=na, later=[nb, nc])


def bad_ones():
    """a bad neighbour and a bad child are skipped for the next; a bad parent is added all the same"""
    m = Map(202)
    a, = m.kf(1)
    bad_n, bad_c, bad_p = m.kf(3, bad=True)
    good_n, good_c, never = m.kf(3)
    m.hold(m.point([a]))
    m.covis(a, [bad_n, good_n, never])
    m.child(a, bad_c)
    m.child(a, good_c)
    m.parent(a, bad_p)
    return m.done(a=a, bad=[bad_n, bad_c], added=[good_n, good_c, bad_p], never=never)


def eleventh():
    """ten covisibles that are bad or already in K1, and an eleventh that could be added"""
    m = Map(203)
    k1 = m.kf(4)
    bad = m.kf(7, bad=True)
    late, = m.kf(1)
    for k in k1:
        m.hold(m.point([k]))
    m.covis(k1[0], k1[1:] + bad + [late])
    return m.done(k1=k1, late=late)


# ---- the votes ------------------------------------------------------------------

def bad_voted():
    """the bad keyframe has the most votes: it is neither in K1 nor the maximum"""
    m = Map(204)
    good, = m.kf(1)
    bad, = m.kf(1, bad=True)
    other, = m.kf(1)
    for p in m.points(5, [bad]):
        m.hold(p)
    for p in m.points(3, [good, bad]):
        m.hold(p)
    m.hold(m.point([other]))
    return m.done(good=good, bad=bad, other=other)


def tie(rank=None):
    """keyframes 1 and 3 tie on the maximum; the order decides"""
    m = Map(205)
    k = m.kf(4)
    for kf, n in zip(k, (1, 3, 2, 3)):
        for p in m.points(n, [kf]):
            m.hold(p)
    m.rank = rank
    return m.done(k=k)


def all_voted_bad():
    m = Map(206)
    bad = m.kf(2, bad=True)
    good, = m.kf(1)
    m.points(4, [good])
    held = [m.point([bad[0]]), m.point(bad)]
    for p in held:
        m.hold(p)
    m.prev = [good]
    return m.done(held=held, good=good)


def no_votes():
    """the frame holds a temporal point, a point without observations and a bad one: nobody votes"""
    m = Map(207)
    a, b, c = m.kf(3)
    m.points(6, [a, b])
    m.points(5, [b])
    m.points(4, [c])
    lone = m.point([c], obs=False)
    badp = m.point([a], bad=True)
    m.hold(lone)
    kp_bad = m.hold(badp)
    m.vo()
    m.free(2)
    m.prev = [b, a]
    return m.done(prev=[b, a], lone=lone, bad=badp, kp_bad=kp_bad)


def long_children(bad_child=None):
    """Child lists of 21, 22 and 90 around the 21 children a walk can take in one look: the first child that can
    be added sits at index 20, at 21 and at 87 (past 21 + 64), behind bad ones, K1 members, children the walk
    appended for an earlier member and the neighbour the same iteration has just appended; a second addable
    child follows at 88.  bad_child=(member, index): that child id lies outside the map."""
    m = Map(209)
    a, b, c = m.kf(3)
    na, nc = m.kf(2)  # the neighbours a and c add first; each is also among the member's own children
    a20, b21, c87, c88 = m.kf(4)
    bad = m.kf(90, bad=True)
    for k in (a, b, c):
        m.hold(m.point([k]))
    for k in (na, nc, a20, b21, c87, c88):
        m.points(3, [k])
    m.covis(a, [na])
    m.covis(c, [nc])
    ca = bad[:20] + [a20]
    ca[3], ca[5], ca[11] = b, na, c  # a K1 member, the neighbour of this iteration, another K1 member
    cb = bad[:21] + [b21]
    cb[0], cb[20] = a20, na  # appended for a
    cc = bad[:87] + [c87, c88, bad[89]]
    cc[2], cc[21], cc[30], cc[84], cc[85], cc[86] = a, b21, nc, a20, b, na
    lists = {a: ca, b: cb, c: cc}
    if bad_child is not None:
        lists["abc".index(bad_child[0])][bad_child[1]] = len(m.bad) + 5
    for k, ch in lists.items():
        for x in ch:
            m.child(k, x)
    return m.done(k1=[a, b, c], added=[na, a20, b21, nc, c87], never=c88, sizes=[len(ca), len(cb), len(cc)])


# ---- points and extras -------------------------------------------------------------

def rich():
    m = Map(208)
    a, b, c = m.kf(3)
    badkf, = m.kf(1, bad=True)
    far, = m.kf(1)  # not local: nothing votes for it and nothing links to it
    m.null(a, 2)
    seen3 = m.point([b, c])  # b slot 0, c slot 0, and a below: its first (position, slot) is a's
    pa = m.points(7, [a])
    m.put(a, seen3)
    m.null(a)
    dead = m.points(3, [a, b], bad=True)  # bad slots are skipped
    pb = m.points(70, [b])
    m.null(c, 3)
    pc = m.points(9, [c, b])
    outside = m.point([far], obs=False)  # held and good, in a keyframe that is not local
    only_bad = m.point([badkf])  # held; the one keyframe it votes for is bad
    twice = m.point([far], obs=False)
    m.points(4, [far])
    names = {"held": [], "culled": [], "extra": [outside, only_bad, twice]}
    for p in pa[:4] + pb[:20] + pc[:3]:
        m.hold(p)
        names["held"].append(p)
    m.free(3)
    kp_bad = m.hold(dead[0])
    for p in pa[4:6] + pb[20:25]:
        m.cull(p)
        names["culled"].append(p)
    m.hold(outside)
    vo1, _ = m.vo()
    kp_twice = m.hold(twice, times=2)
    m.free(1)
    m.hold(only_bad)
    vo2, kp_vo2 = m.vo(times=2)
    m.cull(pb[0])  # matched twice by call 1, culled at one keypoint and kept at another: in row 1, no flag
    m.unused_entries(5)
    return m.done(a=a, b=b, c=c, seen3=seen3, dead=dead, kp_bad=kp_bad, kp_twice=kp_twice, kp_vo2=kp_vo2,
                  vo=[vo1, vo2], **names)


def sized(n_local, n_held, seed=300):
    """n_local local points over four keyframes of 37, 91, 130 .. slots (no multiple of 64; the last takes the
    rest, so a large count crosses the 256-slot tile), every point seen from two keyframes and every fifth
    followed by a NULL slot; n_held keypoints hold local points while there are any and then points outside the
    map's keyframes.  Each keyframe's covisibles are the other three, so with any vote all four are local; with
    none (n_local or n_held 0) the previous list names them."""
    m = Map(seed + 7 * n_local + n_held)
    kfs = m.kf(4)
    for k in kfs:
        m.covis(k, [o for o in kfs if o != k])
    caps = [37, 91, 130]
    pts = []
    while len(pts) < n_local:
        k = next((i for i in range(3) if len(m.slots[kfs[i]]) < caps[i]), 3)
        pts.append(m.point([kfs[k], kfs[(k + 1) % 4]]))
        if len(pts) % 5 == 0:
            m.null(kfs[k])
    lone = m.points(max(n_held - n_local, 0))
    for p in (pts + lone)[:n_held]:
        m.hold(p)
    m.free(2)
    m.prev = kfs
    return m.done(kfs=kfs, pts=pts, lone=lone)


SCENES = {
    "k1_79": lambda: k1_of(79), "k1_80": lambda: k1_of(80), "k1_81": lambda: k1_of(81), "k1_82": lambda: k1_of(82),
    "parent_break": parent_break, "bad_ones": bad_ones, "eleventh": eleventh, "bad_voted": bad_voted,
    "tie": tie, "tie_ranked": lambda: tie(rank=[2, 3, 0, 1]), "all_voted_bad": all_voted_bad, "no_votes": no_votes,
    "rich": rich, "long_children": long_children,
}
