#!/usr/bin/env python3
"""Times the keyframe database on the device on one GPU: 64 relocalisation
queries against 2,000 keyframes of about 1,000 words each (the k=10 / L=6
synthetic vocabulary of the loop-burst leg; keyframes along a looping path over
a landmark pool, ten path neighbours as covisibles) through

  new    orbgpu_kfdb_detect_batch_device: the whole batch in one call, timed
         with device events around it,
  host   the path a caller had before it, as far as the library goes: one
         host-form orbgpu_bow_score call per query over the same keyframes,
         with the CSR packed once beforehand.  The caller's walk of the
         inverted file, its re-pack of the CSR per query and the candidate
         selection on the host are left out, so this is a lower bound.

Medians of --reps calls after --warmup.  Prints one JSON line; --no-host times
the new call alone (for a kernel trace).
"""
import argparse
import ctypes
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "orb-slam2-annotation_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--keypoints", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    import bow
    import kfdb
    import orbgpu
    import synth
    p, l, d, w = synth.synthetic_vocabulary_fast(10, 6, 0x70C)
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "voc.txt"
        synth.write_vocabulary_text_fast(path, 10, 6, 0, 0, p, l, d, w)
        voc = bow.Vocabulary.load_text(str(path))
    leaves = d[l == 1]
    nq, n_kf, S = a.queries, a.keyframes, a.keypoints
    rng = np.random.default_rng(7)
    step = 12
    pool = leaves[rng.integers(0, len(leaves), step * n_kf * 6 // 10)]  # the path comes back after 60 % of it

    def observe(start):
        ids = (start + np.arange(S)) % len(pool)
        return pool[ids] ^ (rng.random((S, 32)) < 0.01).astype(np.uint8)
    dev = torch.device("cuda")
    kf_desc = torch.from_numpy(np.stack([observe(step * k) for k in range(n_kf)])).to(dev)
    q_desc = torch.from_numpy(np.stack([observe(int(s)) for s in rng.integers(0, len(pool), nq)])).to(dev)
    counts_k = torch.full((n_kf,), S, dtype=torch.int32, device=dev)
    counts_q = torch.full((nq,), S, dtype=torch.int32, device=dev)
    tf_k, tf_q = bow.BatchTransform(n_kf, S, dev), bow.BatchTransform(nq, S, dev)
    bow.transform_batch(voc, kf_desc, counts_k, tf_k, 4)
    bow.transform_batch(voc, q_desc, counts_q, tf_q, 4)
    covis = np.full((n_kf, 10), -1, np.int32)
    for k in range(n_kf):
        near = [j for j in sorted(range(max(0, k - 6), min(n_kf, k + 7)), key=lambda j: (abs(j - k), j)) if j != k]
        covis[k, :len(near[:10])] = near[:10]
    db = kfdb.KeyFrameDatabase.from_transform(tf_k, covis, 0)
    db.add(*range(n_kf))
    queries = db.queries([{"kind": kfdb.RELOC, "device": (tf_q.bow_words.data_ptr() + 4 * S * f,
                                                          tf_q.bow_values.data_ptr() + 8 * S * f,
                                                          tf_q.bow_n.data_ptr() + 4 * f)} for f in range(nq)])
    det = kfdb.Detection(nq, n_kf, 16, False, dev)
    db.reserve(nq)
    torch.cuda.synchronize()

    def new():
        db.detect(queries, 16, out=det)

    new()
    torch.cuda.synchronize()
    res = det.query_results()
    n_bow_k, n_bow_q = tf_k.bow_n.cpu().numpy(), tf_q.bow_n.cpu().numpy()
    out = {"queries": nq, "keyframes": n_kf, "words_per_keyframe": float(n_bow_k.mean()),
           "words_per_query": float(n_bow_q.mean()), "statuses": sorted({r.status for r in res}),
           "sharing": float(np.mean([r.n_sharing for r in res])), "scored": float(np.mean([r.n_scored for r in res])),
           "candidates": float(np.mean([r.n_candidates for r in res])), "launches": 5}
    for _ in range(a.warmup):
        new()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        new()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    out["new_ms"] = dict(zip(("median", "min", "max"), (statistics.median(ts), min(ts), max(ts))))
    if a.no_host:
        print(json.dumps(out))
        return
    # the host form over the same keyframes: the CSR packed once
    bw, bv = tf_k.bow_words.cpu().numpy(), tf_k.bow_values.cpu().numpy()
    off = np.zeros(n_kf + 1, np.int32)
    off[1:] = np.cumsum(n_bow_k)
    dw = np.concatenate([bw[k, :n_bow_k[k]] for k in range(n_kf)]).astype(np.int32)
    dv = np.concatenate([bv[k, :n_bow_k[k]] for k in range(n_kf)]).astype(np.float64)
    qw, qv = tf_q.bow_words.cpu().numpy(), tf_q.bow_values.cpu().numpy()
    qws = [np.ascontiguousarray(qw[f, :n_bow_q[f]], np.int32) for f in range(nq)]
    qvs = [np.ascontiguousarray(qv[f, :n_bow_q[f]], np.float64) for f in range(nq)]
    common, scores = np.zeros(n_kf, np.int32), np.zeros(n_kf, np.float64)
    L = orbgpu.lib()
    vp = ctypes.c_void_p
    L.orbgpu_bow_score.argtypes = [ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp]

    def host():
        for f in range(nq):
            orbgpu._check(L.orbgpu_bow_score(0, qws[f].ctypes.data, qvs[f].ctypes.data, len(qws[f]), n_kf,
                                             off.ctypes.data, dw.ctypes.data, dv.ctypes.data, common.ctypes.data,
                                             scores.ctypes.data), "orbgpu_bow_score")

    host()
    det2 = kfdb.Detection(nq, n_kf, 16, True, dev)  # both paths count the same common words (the last query's)
    db.detect(queries, 16, out=det2)
    torch.cuda.synchronize()
    out["common_words_equal"] = bool(np.array_equal(det2.words[nq - 1].cpu().numpy(), common))
    ts = []
    for _ in range(max(3, a.reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["host_ms"] = dict(zip(("median", "min", "max"), (statistics.median(ts), min(ts), max(ts))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
