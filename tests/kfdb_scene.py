"""Scenes for the keyframe database on the device (csrc/kfdb.hip) and the
expected values from oracle/kfdb_ref.py.

The base scene is the looping path of test_adapter._kfdb_scene, restated:
keyframe k sees landmarks [10k, 10k + 250) mod 1200 of a k = 6 / L = 4
vocabulary (about 220 words per BowVector), covisibility = path neighbours.
A scene is a dict:

  scoring, n_words
  kfs         per keyframe {"bow", "connected", "best_covis"}
  in_db       the add() order (a list of keyframe indices); everything else is
              not in the database
  kf_bad      (n_kf,) uint8
  reloc0      (n_kf,) float32: what mRelocScore holds at the call (arbitrary
              finite floats, the reference leaves it uninitialised)

and a query is a dict {"kind", "bow"} plus, for LOOP, "connected", "covisible"
(None: min_score as given) and "min_score".

reference() calls kfdb_ref sequentially in batch order on a fresh copy of the
keyframes and reads its fields back after every query.
"""
from __future__ import annotations

import functools

import numpy as np

import bow_ref
import kfdb_ref
import synth

f32 = np.float32
RELOC, LOOP = 0, 1
COVIS = 10
N_PATH = 130


@functools.lru_cache(maxsize=None)
def _vocabulary(scoring):
    par, leaf, desc, w = synth.synthetic_vocabulary(6, 4, 77)
    return bow_ref.Vocabulary.from_arrays(6, 4, scoring, 0, par, leaf, desc, w), desc[leaf == 1]


@functools.lru_cache(maxsize=None)
def _path(scoring, seed=5):
    """the BowVectors of the whole path (N_PATH keyframes) and of six lost
    frames along it; a scene of n_kf keyframes is a prefix"""
    voc, leaves = _vocabulary(scoring)
    rng = np.random.default_rng(seed)
    lm = leaves[rng.integers(0, len(leaves), 1200)]

    def observe(ids):
        d = lm[ids] ^ (rng.uniform(size=(len(ids), 32)) < 0.03).astype(np.uint8)
        return voc.transform(d, 2)[4]
    bows = []
    for k in range(N_PATH):
        ids = (10 * k + np.arange(250)) % 1200
        bows.append(observe(ids[rng.uniform(size=250) < 0.85]))
    frames = [observe((s + np.arange(250)) % 1200) for s in (500, 35, 260, 515, 45, 1150)]
    return voc.n_words, bows, frames


def neighbours(k, n_kf):
    return [j for j in sorted(range(max(0, k - 6), min(n_kf, k + 7)), key=lambda j: (abs(j - k), j)) if j != k]


def base(scoring, n_kf, seed=5):
    """the looping path with every keyframe add()ed in index order; returns
    (scene, the six relocalisation queries)"""
    n_words, bows, frames = _path(scoring, seed)
    kfs = []
    for k in range(n_kf):
        near = neighbours(k, n_kf)
        kfs.append({"bow": dict(bows[k]), "connected": set(near), "best_covis": near[:COVIS]})
    rng = np.random.default_rng(1000 + n_kf)
    scene = {"scoring": scoring, "n_words": n_words, "kfs": kfs, "in_db": list(range(n_kf)),
             "kf_bad": np.zeros(n_kf, np.uint8), "reloc0": rng.uniform(-0.5, 1.5, n_kf).astype(f32)}
    return scene, [{"kind": RELOC, "bow": dict(b)} for b in frames]


def loop_query(scene, k, covisible=True, min_score=0.0):
    """keyframe k of the scene as LoopClosing::DetectLoop queries it: its
    connected keyframes excluded, minScore from its covisibles (or given)"""
    kf = scene["kfs"][k]
    return {"kind": LOOP, "bow": dict(kf["bow"]), "connected": sorted(kf["connected"]),
            "covisible": sorted(kf["connected"]) if covisible else None, "min_score": min_score}


def covis_rows(scene):
    rows = np.full((len(scene["kfs"]), COVIS), -1, np.int32)
    for k, kf in enumerate(scene["kfs"]):
        rows[k, :len(kf["best_covis"])] = kf["best_covis"]
    return rows


def min_score_of(scene, q):
    """LoopClosing.cpp:136-151: the float 1 lowered by the score against every
    covisible keyframe that is not bad"""
    if q.get("covisible") is None:
        return f32(q["min_score"])
    m = f32(1)
    for c in q["covisible"]:
        if scene["kf_bad"][c]:
            continue
        s = f32(bow_ref.bow_score(scene["scoring"], q["bow"], scene["kfs"][c]["bow"])[0])
        if s < m:
            m = s
    return m


def reference(scene, queries, reloc_start=None):
    """kfdb_ref called once per query in batch order.  Returns (per query a
    dict with the fields of orbgpu_kfdb_result, `candidates`, `words` and
    `scores` (n_kf,), and `stale`, the stale mRelocScore reads it made; the
    final mRelocScore array)."""
    n_kf = len(scene["kfs"])
    kfs = [{"id": k + 1, "bow": kf["bow"], "connected": kf["connected"], "best_covis": kf["best_covis"],
            "loop_query": 0, "loop_words": 0, "loop_score": f32(0), "reloc_query": 0, "reloc_words": 0,
            "reloc_score": f32((scene["reloc0"] if reloc_start is None else reloc_start)[k])}
           for k, kf in enumerate(scene["kfs"])]
    db = kfdb_ref.KeyFrameDatabase(scene["n_words"], scene["scoring"])
    for k in scene["in_db"]:
        db.add(kfs, k)
    out = []
    retain, seen = kfdb_ref._retain, []

    def spy(acc_list, min_keep):  # lAccScoreAndMatch as the reference built it
        seen.append(list(acc_list))
        return retain(acc_list, min_keep)
    kfdb_ref._retain = spy
    try:
        for qi, q in enumerate(queries):
            del seen[:]
            qid = 100000 + qi
            if q["kind"] == RELOC:
                cands = db.detect_reloc(kfs, q["bow"], qid)
                ms, mark, nw, sc = f32(0), "reloc_query", "reloc_words", "reloc_score"
            else:
                ms = min_score_of(scene, q)
                kfs.append({"id": qid, "bow": q["bow"], "connected": set(q["connected"])})  # the query keyframe
                cands = db.detect_loop(kfs, n_kf, ms)
                kfs.pop()
                mark, nw, sc = "loop_query", "loop_words", "loop_score"
            listed = [k for k in range(n_kf) if kfs[k][mark] == qid]
            words = np.zeros(n_kf, np.int32)
            scores = np.zeros(n_kf, f32)
            r = {"n_sharing": len(listed), "max_common": 0, "min_common": 0, "n_filtered": 0, "n_scored": 0,
                 "min_score": ms, "best_acc_score": ms, "stale": 0}
            for k in listed:
                words[k] = kfs[k][nw]
            if listed:
                r["max_common"] = int(words.max())
                r["min_common"] = int(f32(r["max_common"]) * f32(0.8))
                filtered = [k for k in listed if words[k] > r["min_common"]]
                r["n_filtered"] = len(filtered)
                for k in filtered:
                    scores[k] = kfs[k][sc]
                if q["kind"] == RELOC:
                    r["stale"] = sum(1 for k in filtered for j in kfs[k]["best_covis"]
                                     if kfs[j][mark] == qid and words[j] <= r["min_common"])
            if seen:
                r["n_scored"] = len(seen[0])
                r["best_acc_score"] = max([ms] + [a for a, _ in seen[0]])
                r["acc_list"] = seen[0]
            r.update(candidates=[int(c) for c in cands], n_candidates=len(cands), words=words, scores=scores)
            out.append(r)
    finally:
        kfdb_ref._retain = retain
    return out, np.array([kfs[k]["reloc_score"] for k in range(n_kf)], f32)
