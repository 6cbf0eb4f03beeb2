"""Sequential restatement of the covisibility table's one call (include/orbgpu_covis.h,
csrc/covis.hip), written from the reference's lines: the graph part of
KeyFrame::SetBadFlag (src/KeyFrame.cpp:572-573, :584-585) with EraseConnection
(:677-691) and UpdateBestCovisibles (:161-184).  Plain Python, one keyframe after
another.
"""
from __future__ import annotations

OK, BAD_JOB = 0, 3
BEST = 10


def best_covisibles(row):
    """UpdateBestCovisibles (:161-184): sort on (weight, KeyFrame*) ascending, then reversed.  The row is in map
    order, so the position in it stands for the pointer."""
    pairs = sorted((w, i) for i, (_, w) in enumerate(row))
    return [row[i] for _, i in reversed(pairs)]


class Table:
    """the graph: per keyframe conn (mConnectedKeyFrameWeights in map order) and ord
    (mvpOrderedConnectedKeyFrames with mvOrderedWeights) as lists of (keyframe, weight)"""

    def __init__(self, n_kf, stride, conn=None, ord=None):
        """conn: keyframe -> its row in map order; ord: keyframe -> an ordered row to hold in place of the one
        that follows from conn"""
        self.n_kf, self.stride = n_kf, stride
        self.conn = [list(conn.get(k, [])) if conn else [] for k in range(n_kf)]
        self.ord = [list(ord[k]) if ord and k in ord else best_covisibles(c) for k, c in enumerate(self.conn)]

    def covis10(self, k):
        best = [kf for kf, _ in self.ord[k][:BEST]]
        return best + [-1] * (BEST - len(best))


def erase_keyframes(T, kfs):
    """the graph part of SetBadFlag for kfs in order, on the table T, which it changes; returns the statuses"""
    out = []
    for x in kfs:
        if not 0 <= x < T.n_kf:
            out.append(BAD_JOB)
            continue
        for nb, _ in list(T.conn[x]):  # :572-573
            if 0 <= nb < T.n_kf and nb != x and any(k == x for k, _ in T.conn[nb]):  # :682
                T.conn[nb] = [e for e in T.conn[nb] if e[0] != x]
                T.ord[nb] = best_covisibles(T.conn[nb])  # :689-690
        T.conn[x], T.ord[x] = [], []  # :584-585
        out.append(OK)
    return out
