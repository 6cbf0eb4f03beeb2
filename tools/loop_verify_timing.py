#!/usr/bin/env python3
"""Times the verified loop of LoopClosing::ComputeSim3 on one GPU: the burst of
bench.py's loop leg (100 queries x 5 candidates, 1000 keypoints, 40 % true
correspondences and 60 % geometric outliers, the k=10 / L=6 vocabulary) with
keypoints and distance ranges added (tests/loop_verify_scene.py), through

  new    orbgpu_compute_sim3_verified_batch_device: every pass of every query
         enqueued in one call (as many passes as the burst needs, found first),
  chain  what a caller had before it: orbgpu_compute_sim3_batch_device, a
         synchronise, then per matched query the host forms
         orbgpu_search_by_sim3 and orbgpu_optimize_sim3_batch (marshalled from
         Python, so the figure includes that cost), which verifies only the
         first return of each query.

SearchByBoW and the Sim3Solver set-up run before both and are not timed.
Medians of --reps calls after --warmup, a host clock around work that ends in a
device synchronise.  Prints one JSON line.
"""
import argparse
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
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--cands", type=int, default=5)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    import bow
    import loop
    import loop_verify_scene as lvs
    import proj
    import sim3opt
    import synth
    from lm_ref import quat_from_R
    p, l, d, w = synth.synthetic_vocabulary_fast(10, 6, 0x70C)
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "voc.txt"
        synth.write_vocabulary_text_fast(path, 10, 6, 0, 0, p, l, d, w)
        voc = bow.Vocabulary.load_text(str(path))
    nq, nc = a.queries, a.cands
    sc = lvs.build(nq, nc, n_kp=a.keypoints, inlier_frac=0.4, outlier_frac=0.6, seed=55, leaves=d[l == 1],
                   oracle_bow=False)
    kfs = loop.Keyframes(sc["desc"], sc["angle"], sc["octave"], sc["valid"], sc["mp_world"], sc["Tcw"], sc["K"],
                         sc["sigma2"])
    kfs.compute_bow(voc)
    ks = loop.KeyframeSearch(kfs, sc["kps"], sc["mp_desc"], sc["min_dist"], sc["max_dist"], lvs.BOUNDS, lvs.SF,
                             sc["inv_level_sigma2"], lvs.LOG_SF, sc["Tcw"], sc["K"])
    lb = loop.LoopBurst(kfs, [(cur, cands, 1000 + q) for q, (cur, cands) in enumerate(sc["queries"])], search=ks)
    passes = lb.step_verified(n_passes=1)  # SearchByBoW, the set-up, and how many passes the burst needs
    torch.cuda.synchronize()
    res = lb.verified_results()
    out = {"queries": nq, "cands": nc, "keypoints": a.keypoints, "passes": passes,
           "matched": sum(r.status == loop.MATCHED for r in res),
           "verifications": sum(r.verifications for r in res)}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def new():
        lb.compute_sim3_verified(passes)
        torch.cuda.synchronize()

    match12 = lb.match.cpu().numpy()
    K = sc["K"]

    def chain():
        lb.compute_sim3()
        torch.cuda.synchronize()
        old = lb.query_results()
        n_ok = 0
        for q, r in enumerate(old):
            if r.matched < 0:
                continue
            cur, cands = sc["queries"][q]
            kf = cands[r.matched]
            vb = lb.vb_inliers(q, old)
            m = np.where(vb, match12[q * nc + r.matched], -1)
            v1, v2 = sc["valid"][cur].astype(bool), sc["valid"][kf].astype(bool)
            named = np.zeros(len(v2), bool)
            named[m[m >= 0]] = True
            R12, t12, s12 = np.array(r.R12, np.float32), np.array(r.t12, np.float32), np.float32(r.s12)
            _, agreed = proj.search_by_sim3(lvs.kf_target(sc, cur), lvs.kf_target(sc, kf),
                                            lvs.kf_points(sc, cur, (v1 & (m < 0)).astype(np.int32)),
                                            lvs.kf_points(sc, kf, (v2 & ~named).astype(np.int32)), s12, R12, t12, 7.5)
            m = np.where(agreed >= 0, agreed, m)
            g = np.nonzero((m >= 0) & v1)[0]
            g = g[v2[m[g]]]
            i2 = m[g]
            R1, t1 = sc["Tcw"][cur, :9].reshape(3, 3), sc["Tcw"][cur, 9:]
            R2, t2 = sc["Tcw"][kf, :9].reshape(3, 3), sc["Tcw"][kf, 9:]
            P1c = (sc["mp_world"][cur][g].astype(np.float64) @ R1.T.astype(np.float64)).astype(np.float32) + t1
            P2c = (sc["mp_world"][kf][i2].astype(np.float64) @ R2.T.astype(np.float64)).astype(np.float32) + t2
            k1, k2 = sc["kps"][cur], sc["kps"][kf]
            q12 = quat_from_R(R12.reshape(3, 3).astype(np.float64).tolist())
            n_in, _, _, _ = sim3opt.optimize_sim3(
                q12, t12.astype(np.float64), float(s12), P1c, P2c, np.stack([k1["x"][g], k1["y"][g]], 1),
                np.stack([k2["x"][i2], k2["y"][i2]], 1), sc["inv_level_sigma2"][k1["octave"][g]],
                sc["inv_level_sigma2"][k2["octave"][i2]], K, K, 10.0, False)
            n_ok += n_in >= 20
        return n_ok

    out["new_ms"] = dict(zip(("median", "min", "max"), timed(new)))
    out["chain_ms"] = dict(zip(("median", "min", "max"), timed(chain)))
    out["chain_verified"] = int(chain())

    def ransac_only():
        lb.compute_sim3()
        torch.cuda.synchronize()

    out["compute_sim3_only_ms"] = dict(zip(("median", "min", "max"), timed(ransac_only)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
