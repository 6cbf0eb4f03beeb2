"""Small constructed maps for the gather of Optimizer::LocalBundleAdjustment
(csrc/localba_map.hip, tests/localba_map_ref.py), in the manner of
localmap_scene.py: a scene is built from named keyframes and points, and the
names come back so a test can assert on what each is there to show.

``Map`` builds the mirror pair (include/orbgpu_localmap.h and
include/orbgpu_localba_map.h) by hand:

  kf(n, bad, first)          n keyframes with random poses; returns their indices
  point(bad)                 a map point with a random position
  slot(kf, p, stereo)        a fresh keypoint of kf holding p (-1: NULL); returns
                             its index.  stereo=False: mvuRight negative
  observe(p, kf, idx)        p lists an observation (kf, idx), after its others
  see(kf, p, stereo)         slot + observe: the ordinary case
  covis(kf, others)          GetVectorCovisibleKeyFrames()

Keypoints, poses and positions are random: the gather copies them.  ``SCENES``
names the constructed cases, ``sized`` makes the edge sizes and ``from_problem``
turns a tests/test_localba.py scene into a map whose gathered job is that scene.
"""
from __future__ import annotations

import numpy as np

VALID, HAS_OBS = 1, 2
F32 = np.float32
SIGMA = (1.0 / 1.2 ** (2.0 * np.arange(8))).astype(F32)  # mvInvLevelSigma2


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
        self.bad, self.first, self.Tcw, self.cam = [], [], [], []
        self.slots, self.kp, self.sig, self.cov = [], [], [], []
        self.pt_bad, self.pos, self.obs, self.idx = [], [], [], []

    def kf(self, n=1, bad=False, first=False):
        start = len(self.bad)
        for _ in range(n):
            self.bad.append(int(bad))
            self.first.append(int(first))
            q, _ = np.linalg.qr(self.rng.normal(size=(3, 3)))
            q *= np.sign(np.linalg.det(q))  # a rotation, so a job gathered here is one LBA can take
            self.Tcw.append(np.hstack([q, self.rng.normal(size=(3, 1))]).astype(F32).reshape(12))
            self.cam.append((np.array([517.3, 516.5, 318.6, 255.3, 40.0]) + self.rng.normal(size=5)).astype(F32))
            self.slots.append([])
            self.kp.append([])
            self.sig.append([])
            self.cov.append([])
        return list(range(start, start + n))

    def point(self, bad=False):
        self.pt_bad.append(bool(bad))
        self.pos.append(self.rng.normal(size=3).astype(F32))
        self.obs.append([])
        self.idx.append([])
        return len(self.pt_bad) - 1

    def slot(self, kf, p=-1, stereo=False):
        x, y = self.rng.uniform(0, 640), self.rng.uniform(0, 480)
        ur = self.rng.uniform(1, 600) if stereo else -float(self.rng.integers(1, 4))  # any negative is monocular
        self.slots[kf].append(int(p))
        self.kp[kf].append((x, y, ur))
        self.sig[kf].append(SIGMA[self.rng.integers(0, 8)])
        return len(self.slots[kf]) - 1

    def observe(self, p, kf, idx):
        self.obs[p].append(int(kf))
        self.idx[p].append(int(idx))

    def see(self, kf, p, stereo=False):
        i = self.slot(kf, p, stereo)
        self.observe(p, kf, i)
        return i

    def covis(self, kf, others):
        self.cov[kf] = [int(v) for v in others]

    def build(self, kf, names=None):
        n_kf, n_pt, rng = len(self.bad), len(self.pt_bad), self.rng
        cov10 = np.full((n_kf, 10), -1, np.int32)
        for k, c in enumerate(self.cov):
            cov10[k, :min(len(c), 10)] = c[:10]
        flags = np.array([(0 if b else VALID) | (HAS_OBS if o else 0) for b, o in zip(self.pt_bad, self.obs)], np.int32)
        mirror = {"kf_bad": np.array(self.bad, np.uint8), "slots": [np.array(s, np.int32) for s in self.slots],
                  "covis": cov10, "children": [[] for _ in range(n_kf)], "parent": np.full(n_kf, -1, np.int32),
                  "kf_by_rank": None, "pt_flags": flags.reshape(n_pt), "obs": [list(o) for o in self.obs],
                  "pos": np.array(self.pos, F32).reshape(n_pt, 3), "normal": rng.normal(size=(n_pt, 3)).astype(F32),
                  "desc": rng.integers(0, 256, (n_pt, 32), dtype=np.uint8), "min_dist": np.ones(n_pt, F32),
                  "max_dist": np.full(n_pt, 9, F32)}
        ba = {"covis_all": [list(c) for c in self.cov], "kf_first": np.array(self.first, np.uint8),
              "kf_Tcw": np.array(self.Tcw, F32).reshape(n_kf, 12), "kf_cam": np.array(self.cam, F32).reshape(n_kf, 5),
              "kp_obs": [np.array(k, F32).reshape(-1, 3) for k in self.kp],
              "kp_inv_sigma2": [np.array(s, F32).reshape(-1) for s in self.sig], "obs_idx": [list(i) for i in self.idx]}
        return _freeze({"mirror": mirror, "ba": ba, "kf": int(kf), "names": names or {}})


# ---- the named scenes -----------------------------------------------------------------------------------

def rich():
    """pKF `a` with the covisibles b, a bad one (cb) and c; the fixed cameras e, d and f0 (the map's first
    keyframe), a bad fixed observer (fb), a keyframe nobody local sees (far)"""
    m = Map(11)
    f0, = m.kf(first=True)
    far, a, b = m.kf(3)
    cb, = m.kf(bad=True)
    c, d, e = m.kf(3)
    fb, = m.kf(bad=True)
    m.covis(a, [b, cb, c])
    m.covis(b, [a, far])  # b's own list is not read
    # p0: an early point whose LAST observation is the first sight of e; p1's FIRST observation is d's
    p0 = m.point()
    m.see(a, p0)
    m.see(b, p0, stereo=True)
    m.see(e, p0)
    p1 = m.point()
    m.see(d, p1, stereo=True)
    m.see(a, p1)
    m.slot(a)  # NULL
    dead = m.point(bad=True)
    m.see(a, dead)
    m.see(b, dead)
    # mono and stereo interleaved in one point, over local and fixed cameras; cb and fb see it too
    mix = m.point()
    for k, st in ((a, False), (cb, True), (b, True), (c, False), (fb, False), (d, True), (e, False)):
        m.see(k, mix, stereo=st)
    # a point without observations, in pKF's slot
    lonely = m.point()
    m.slot(a, lonely)
    own = []
    for i in range(5):
        p = m.point()
        own.append(p)
        m.see(a, p, stereo=bool(i & 1))
        m.see(cb, p)  # the bad covisible observes local points
        if i < 2:
            m.see(fb, p)
    # `early` sits in b's slot 5 and in c's slot 1: b is listed before c, so the walk finds it in b, after
    # `tail` in b's slot 4 -- the later-listed keyframe's lower slot number does not decide
    m.slot(b)
    early = m.point()
    tail = m.point()
    m.see(c, early)
    m.see(b, tail)
    m.see(b, early)
    # found in b's slot `held`, observed from b at the keypoint `shifted`, a NULL slot
    shift = m.point()
    held = m.slot(b, shift)
    shifted = m.slot(b, -1, stereo=True)
    m.observe(shift, b, shifted)
    # in c's slot, but its only observation is f0's: local through the slot, no edge from c
    ghost = m.point()
    m.slot(c, ghost)
    m.see(f0, ghost)
    c_own = m.point()
    m.see(c, c_own, stereo=True)
    m.see(far, m.point())  # not local: far is in nobody's list that is read
    return m.build(a, dict(a=a, b=b, c=c, cb=cb, d=d, e=e, f0=f0, fb=fb, far=far, p0=p0, p1=p1, dead=dead, mix=mix,
                           lonely=lonely, own=own, early=early, tail=tail, shift=shift, held=held, shifted=shifted,
                           ghost=ghost, c_own=c_own))


def bad_pkf():
    """pKF is bad: listed first all the same (:544), its points are local, and no edge is its own (:688)"""
    m = Map(12)
    a, = m.kf(bad=True)
    b, d = m.kf(2)
    m.covis(a, [b])
    pts = [m.point() for _ in range(4)]
    for i, p in enumerate(pts):
        m.see(a, p, stereo=bool(i & 1))
        if i < 3:
            m.see(b, p)
        if i >= 2:
            m.see(d, p, stereo=True)
    return m.build(a, dict(a=a, b=b, d=d, pts=pts))


def first_local():
    """the map's first keyframe is a covisible of pKF: a local pose with its fixed flag set (:624)"""
    m = Map(13)
    k0, = m.kf(first=True)
    a, d = m.kf(2)
    m.covis(a, [k0])
    for i in range(3):
        p = m.point()
        m.see(a, p)
        m.see(k0, p, stereo=True)
        m.see(d, p)
    return m.build(a, dict(a=a, k0=k0, d=d))


def empty():
    """pKF holds nothing and has no covisible: one pose, no point, no edge"""
    m = Map(14)
    a, b = m.kf(2)
    m.slot(a)
    m.see(b, m.point())
    return m.build(a, dict(a=a, b=b))


def dup_covis():
    """outside the caller's contract: covis_all names b twice and pKF itself; the first occurrence is kept"""
    m = Map(15)
    a, b, c = m.kf(3)
    m.covis(a, [b, a, c, b])
    for k in (a, b, c):
        p = m.point()
        m.see(k, p)
    return m.build(a, dict(a=a, b=b, c=c))


SCENES = {"rich": rich, "bad_pkf": bad_pkf, "first_local": first_local, "empty": empty, "dup_covis": dup_covis}


# ---- the edge sizes ------------------------------------------------------------------------------------

def sized(n_covis=2, n_points=6, n_obs0=None, n_fixed=2, nulls=1, seed=20):
    """pKF with n_covis covisibles (every seventh bad), n_points points in its slots after `nulls` NULL ones
    (pKF has n_points + nulls slots), n_fixed fixed cameras each seen by the point f % n_points.  n_obs0: the
    exact length of point 0's observation list (0: none at all), filled up from the covisibles and then from
    fresh fixed cameras."""
    m = Map(seed)
    a, = m.kf()
    cov = [m.kf(bad=(i % 7 == 3))[0] for i in range(n_covis)]
    fix = [m.kf()[0] for _ in range(n_fixed)]
    m.covis(a, cov)
    for _ in range(nulls):
        m.slot(a)
    pts = [m.point() for _ in range(n_points)]
    for j, p in enumerate(pts):
        if j == 0 and n_obs0 is not None:
            i = m.slot(a, p)
            want = [a] + cov + fix[0::max(n_points, 1)]
            want += [m.kf()[0] for _ in range(n_obs0 - len(want))]
            for q, k in enumerate(want[:n_obs0]):
                m.observe(p, k, i) if k == a else m.see(k, p, stereo=bool(q & 1))
            continue
        m.see(a, p, stereo=bool(j % 3 == 1))
        for f in fix[j::n_points]:
            m.see(f, p, stereo=bool(f & 1))
    return m.build(a, dict(a=a, cov=cov, fix=fix, pts=pts))


# ---- a tests/test_localba.py scene as a map ---------------------------------------------------------------

def from_problem(s):
    """The mirror pair and pKF of a synth.localba_scene: keyframe i is pose i, point j is point j, pKF is
    pose 0 and the other local poses are its covisibles in order; every keyframe's slots hold the points it
    observes, ascending, and a point's observations are its edges in the scene's order.  A gathered job
    equals the scene up to the documented orders: the points in first-seen order over the local keyframes'
    slots, the fixed poses in first-sight order."""
    sc = from_problems([s])
    return dict(sc, kf=sc["kfs"][0])


def from_problems(scenes):
    """several such scenes side by side in one map, each with keyframes and points of its own; `kfs` lists
    their pKFs"""
    m = Map(0)
    kfs = []
    for s in scenes:
        P, M, NL = len(s["Tcw"]), len(s["Xw"]), int(s["n_local"])
        k0, j0 = len(m.bad), len(m.pt_bad)
        kfs.append(k0)
        m.kf(P)
        for i in range(P):
            m.first[k0 + i] = int(s["fixed"][i]) if i < NL else 0
            m.Tcw[k0 + i] = np.asarray(s["Tcw"][i], F32).reshape(-1, 4)[:3].reshape(12)
            m.cam[k0 + i] = np.asarray(s["cam"][i], F32)
        m.covis(k0, range(k0 + 1, k0 + NL))
        for j in range(M):
            m.point()
            m.pos[j0 + j] = np.asarray(s["Xw"][j], F32)
        for e in range(len(s["pose_idx"])):
            k, j = k0 + int(s["pose_idx"][e]), j0 + int(s["point_idx"][e])
            m.slots[k].append(j)
            m.kp[k].append(tuple(s["obs"][e]))
            m.sig[k].append(s["inv_sigma2"][e])
            m.observe(j, k, len(m.slots[k]) - 1)
    return dict(m.build(kfs[0]), kfs=kfs)
