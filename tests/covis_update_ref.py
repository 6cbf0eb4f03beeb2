"""Sequential restatement of KeyFrame::UpdateConnections and of LocalMapping::KeyFrameCulling on the
covisibility table (include/orbgpu_covis.h, csrc/covis.hip), written from the reference's lines:
UpdateConnections (src/KeyFrame.cpp:369-483) with AddConnection (:140-154) and UpdateBestCovisibles
(:161-184); KeyFrameCulling (src/LocalMapping.cpp:802-880) with KeyFrame::SetBadFlag (src/KeyFrame.cpp:559-585),
MapPoint::EraseObservation (src/MapPoint.cpp:141-169) and the NULLing of a bad point's slots.  Plain Python on
covis_ref.Table, one keyframe after another.  The culling holds a real SetBadFlag on a copy of the scene's
observations -- not the device's overlay, which is tested against it.

``Scene`` is a small map built by hand: keyframes with slots (point id, octave, mvuRight sign, depth), points
with their observation maps, and the order that stands for the std::map's.
"""
from __future__ import annotations

import numpy as np

import covis_ref as cr

OK, EMPTY, CAPACITY, BAD_JOB = 0, 1, 2, 3
KEPT, CULLED, TO_BE_ERASED, SKIPPED_FIRST = 0, 1, 2, 3
TH = 15


class Scene:
    def __init__(self, n_kf, kf_by_rank=None):
        self.n_kf, self.kf_by_rank = n_kf, kf_by_rank
        self.slots = [[] for _ in range(n_kf)]     # point id or -1
        self.octave = [[] for _ in range(n_kf)]    # mvKeysUn[s].octave
        self.stereo = [[] for _ in range(n_kf)]    # mvuRight[s] >= 0
        self.depth = [[] for _ in range(n_kf)]     # mvDepth[s]
        self.th_depth = [35.0] * n_kf
        self.not_erase = [0] * n_kf
        self.first = [0] * n_kf
        self.pt_valid, self.obs, self.idx = [], [], []

    def point(self, valid=True):
        self.pt_valid.append(bool(valid))
        self.obs.append([])
        self.idx.append([])
        return len(self.pt_valid) - 1

    def slot(self, kf, p=-1, octave=0, stereo=False, depth=1.0):
        """a fresh keypoint of kf that holds p, without an observation"""
        self.slots[kf].append(int(p))
        self.octave[kf].append(int(octave))
        self.stereo[kf].append(bool(stereo))
        self.depth[kf].append(float(np.float32(depth)))  # the float the mirror holds
        return len(self.slots[kf]) - 1

    def see(self, kf, p, **kw):
        """slot + observation: the ordinary case"""
        s = self.slot(kf, p, **kw)
        self.obs[p].append(int(kf))
        self.idx[p].append(s)
        return s

    def rank_of(self):
        order = list(range(self.n_kf)) if self.kf_by_rank is None else list(self.kf_by_rank)
        rank = [0] * self.n_kf
        for r, k in enumerate(order):
            rank[k] = r
        return rank

    def job_is_bad(self, x):
        """an index that UpdateConnections of x reads lies outside the map"""
        if not 0 <= x < self.n_kf:
            return True
        for p in self.slots[x]:
            if p == -1:
                continue
            if not 0 <= p < len(self.pt_valid):
                return True
            if self.pt_valid[p] and any(not 0 <= k < self.n_kf for k in self.obs[p]):
                return True
        return False


def add_connection(T, rank_of, nb, key, w):
    """nb->AddConnection(key, w) (:140-154)"""
    row = T.conn[nb]
    at = [i for i, (k, _) in enumerate(row) if k == key]
    if not at:
        place = sum(1 for k, _ in row if 0 <= k < T.n_kf and rank_of[k] < rank_of[key])  # the std::map's order
        row.insert(place, (key, w))
    elif row[at[0]][1] != w:
        row[at[0]] = (key, w)
    else:
        return  # :149-150
    T.ord[nb] = cr.best_covisibles(row)


def update_connections(T, S, kfs):
    """UpdateConnections for kfs in order on the table T, which it changes; returns per keyframe the dict
    {status, n_counted, n_ordered, kf_max, w_max, front}"""
    rank_of, out = S.rank_of(), []
    res = lambda status, nc=0, no=0, km=-1, wm=0, front=-1: dict(status=status, n_counted=nc, n_ordered=no, kf_max=km,
                                                                  w_max=wm, front=front)
    for x in kfs:
        if S.job_is_bad(x):
            out.append(res(BAD_JOB))
            continue
        counter = {}
        for p in S.slots[x]:  # :388-408
            if p == -1 or not S.pt_valid[p]:
                continue
            for k in S.obs[p]:
                if k != x:
                    counter[k] = counter.get(k, 0) + 1
        if not counter:  # :411
            out.append(res(EMPTY))
            continue
        items = sorted(counter.items(), key=lambda kv: rank_of[kv[0]])  # the std::map's order
        nmax, kmax, pairs = 0, None, []
        for k, w in items:  # :425-441
            if w > nmax:
                nmax, kmax = w, k
            if w >= TH:
                pairs.append((w, k))
        if not pairs:  # :444-451
            pairs = [(nmax, kmax)]
        full = lambda k: all(e[0] != x for e in T.conn[k]) and len(T.conn[k]) >= T.stride
        if len(items) > T.stride or any(full(k) for _, k in pairs):
            out.append(res(CAPACITY, len(items), len(pairs), kmax, nmax))
            continue
        for w, k in pairs:
            add_connection(T, rank_of, k, x, w)
        pairs.sort(key=lambda wk: (wk[0], rank_of[wk[1]]))  # :454, on (weight, KeyFrame*)
        T.conn[x] = items  # :469
        T.ord[x] = [(k, w) for w, k in reversed(pairs)]  # :457-471
        out.append(res(OK, len(items), len(pairs), kmax, nmax, T.ord[x][0][0]))
    return out


class LiveMap:
    """a copy of a Scene's slots and observations that SetBadFlag changes"""

    def __init__(self, S):
        self.S = S
        self.slots = [list(s) for s in S.slots]
        self.bad = [not v for v in S.pt_valid]
        self.obs = [dict(zip(o, i)) for o, i in zip(S.obs, S.idx)]
        self.n_obs = [sum(2 if S.stereo[k][s] else 1 for k, s in o.items()) for o in self.obs]  # AddObservation

    def erase_observation(self, p, kf):
        """MapPoint::EraseObservation (MapPoint.cpp:141-169), and MapPoint::SetBadFlag's NULLing of the slots"""
        if kf not in self.obs[p]:
            return
        self.n_obs[p] -= 2 if self.S.stereo[kf][self.obs[p][kf]] else 1
        del self.obs[p][kf]
        if self.n_obs[p] <= 2:  # :162
            self.bad[p] = True
            for k, s in self.obs[p].items():
                self.slots[k][s] = -1
            self.obs[p] = {}

    def set_bad_flag(self, kf):
        """KeyFrame::SetBadFlag's EraseObservation loop (KeyFrame.cpp:575-577)"""
        for p in list(self.slots[kf]):
            if p != -1:
                self.erase_observation(p, kf)


def keyframe_culling(T, S, kf, mono, set_bad=True):
    """the judging loop for mpCurrentKeyFrame = kf on a LiveMap of S; T is read only.  Returns (result dict,
    verdict rows [(kf, n_mps, n_redundant, verdict)], the culled keyframes in list order).  set_bad=False leaves
    SetBadFlag out: every entry judged on the map as it stands, to show which verdicts the erasures change"""
    L, rows, culled, n_tbe = LiveMap(S), [], [], 0
    for k, _ in list(T.ord[kf]):  # :810
        if S.first[k]:  # :816
            rows.append((k, 0, 0, SKIPPED_FIRST))
            continue
        n_mps = n_red = 0
        for s, p in enumerate(L.slots[k]):
            if p == -1 or L.bad[p]:
                continue
            if not mono and (S.depth[k][s] > S.th_depth[k] or S.depth[k][s] < 0):  # :837
                continue
            n_mps += 1
            if L.n_obs[p] > 3:  # :843
                level = S.octave[k][s]
                seen = sum(1 for ki, si in L.obs[p].items() if ki != k and S.octave[ki][si] <= level + 1)
                n_red += seen >= 3
        verdict = KEPT
        if float(n_red) > 0.9 * float(n_mps):  # :877
            if S.not_erase[k]:  # KeyFrame.cpp:565-569
                verdict, n_tbe = TO_BE_ERASED, n_tbe + 1
            else:
                verdict = CULLED
                culled.append(k)
                if set_bad:
                    L.set_bad_flag(k)
        rows.append((k, n_mps, n_red, verdict))
    return dict(status=OK, n_list=len(rows), n_culled=len(culled), n_to_be_erased=n_tbe), rows, culled


# ---- a looping path --------------------------------------------------------------------------------------

def looping_scene(n_kf, seed, loops=2, pts_per_kf=12, span=6, stereo_every=3):
    """a camera that goes `loops` times round a ring of places: keyframe k stands at place k mod (n_kf / loops)
    and sees the points of the places near it, so keyframes of different rounds are covisible and many are
    redundant.  Returns (Scene, conn rows of every keyframe from UpdateConnections in index order)"""
    rng = np.random.default_rng(seed)
    S = Scene(n_kf)
    S.first[0] = 1
    places = max(1, n_kf // loops)
    pts = [[S.point() for _ in range(pts_per_kf)] for _ in range(places)]
    for k in range(n_kf):
        here = k % places
        for d in range(-span, span + 1):
            for p in pts[(here + d) % places]:
                if rng.random() < 0.75 - 0.08 * abs(d):
                    S.see(k, p, octave=int(rng.integers(0, 4)), stereo=(k % stereo_every == 0),
                          depth=float(rng.uniform(0.5, 50.0)))
    T = cr.Table(n_kf, 1)
    T.stride = n_kf
    update_connections(T, S, list(range(n_kf)))
    T.stride = max(1, max(len(r) for r in T.conn))
    return S, T
