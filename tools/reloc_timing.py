#!/usr/bin/env python3
"""Times Tracking::Relocalization's candidate loop on one GPU: a burst of lost
frames (64 x 5 candidate keyframes, 1000 keypoints, the k=10 / L=6 vocabulary;
per frame two false candidates, one that returns a pose and fails its
verification, one whose row is cut to 30 pairs so that it needs the projection
search, and one that passes at once, tests/reloc_scene.py) through

  new    orbgpu_relocalize_batch_device: every pass of every query enqueued in
         one call (as many passes as the burst needs, found first),
  host   what a caller had before it, frame by frame through the host entries:
         orbgpu_pnp_ransac_batch per iterate() with the draws made on the host,
         orbgpu_pose_optimization_batch and orbgpu_search_by_projection per
         verification stage, each a synchronising call (marshalled from
         Python, so the figure includes that cost).

SearchByBoW and the PnPsolver set-up run before both and are not timed.
Medians of --reps calls after --warmup, a host clock around work that ends in a
device synchronise.  Prints one JSON line; --no-host times the new call alone
(for a kernel trace).
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

FALSE = [dict(n=60, row=True, garbage=True)]
RETURNS = [dict(n=30, row=True), dict(n=30, row=True, garbage=True)]
SEARCHES = [dict(n=120, row=True)]
PASSES = [dict(n=300, row=True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    import bow
    import loop
    import poseopt
    import proj
    import ransac
    import reloc
    import reloc_scene as rs
    import synth
    p, l, d, w = synth.synthetic_vocabulary_fast(10, 6, 0x70C)
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "voc.txt"
        synth.write_vocabulary_text_fast(path, 10, 6, 0, 0, p, l, d, w)
        voc = bow.Vocabulary.load_text(str(path))
    nq, S = a.queries, a.keypoints
    cands = [FALSE, RETURNS, FALSE, SEARCHES, PASSES]
    nc = len(cands)
    sc = rs.build(cands, seed=77, n_queries=nq, n_kp=S, leaves=d[l == 1], oracle_bow=False)
    frames = reloc.Frames(sc["f_kps"], sc["f_desc"], None, sc["K"], 0.0, rs.BOUNDS, rs.SF, sc["sigma2"],
                          sc["inv_level_sigma2"], rs.LOG_SF)
    kfs = loop.Keyframes(sc["desc"], sc["angle"], sc["octave"], sc["valid"], sc["mp_world"], sc["Tcw"], sc["K"],
                         sc["sigma2"])
    frames.compute_bow(voc)
    kfs.compute_bow(voc)
    ks = loop.KeyframeSearch(kfs, sc["kps"], sc["mp_desc"], sc["min_dist"], sc["max_dist"], rs.BOUNDS, rs.SF,
                             sc["inv_level_sigma2"], rs.LOG_SF, sc["Tcw"], sc["K"])
    rb = reloc.RelocBurst(frames, kfs, ks, [(f, c, 1000 + q) for q, (f, c) in enumerate(sc["queries"])])
    rb.search_by_bow()
    row = rb.match.view(nq, nc, S)[:, 3]  # the searching candidate's row keeps its first 30 pairs
    row[(row >= 0).cumsum(1) > 30] = -1
    rb.nmatches.view(nq, nc)[:, 3] = (row >= 0).sum(1).to(torch.int32)
    rb.setup()
    passes = 0  # how many passes the burst needs
    while passes == 0 or any(r.status == reloc.PENDING for r in rb.query_results()):
        rb.relocalize(1, resume=passes > 0)
        passes += 1
    torch.cuda.synchronize()
    res = rb.query_results()
    out = {"queries": nq, "cands": nc, "keypoints": S, "passes": passes,
           "matched": sum(r.status == reloc.MATCHED for r in res), "calls": sum(r.calls for r in res),
           "verifications": sum(r.verifications for r in res), "hypotheses": sum(r.hypotheses for r in res),
           "launches_per_pass": {"schedule": 1, "pnp": 2, "after_pnp": 1, "poseopt": 3, "proj": 2, "stage": 5}}

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(zip(("median", "min", "max"), (statistics.median(ts), min(ts), max(ts))))

    def new():
        rb.relocalize(passes)
        torch.cuda.synchronize()

    out["new_ms"] = timed(new, a.reps)
    if a.no_host:
        print(json.dumps(out))
        return

    match, nmatches = rb.match.cpu().numpy(), rb.nmatches.cpu().numpy()
    K, inv_s2 = sc["K"], sc["inv_level_sigma2"]

    def optimise(f, kf, mp, T, outlier):
        k = sc["f_kps"][f]
        g = np.nonzero(mp >= 0)[0]
        obs = np.stack([k["x"][g], k["y"][g], np.full(len(g), -1.0, np.float32)], 1)
        T, o, n_good = poseopt.pose_optimization(T, sc["mp_world"][kf][mp[g]], obs, inv_s2[k["octave"][g]], K, 0.0)
        outlier[g] = o
        return T, n_good

    def search(f, kf, mp, found, T, th, orb_dist):
        flags = (sc["valid"][kf].astype(bool) & ~found).astype(np.int32)
        return proj.search_by_projection(proj.KEYFRAME, rs.frame_target(sc, f, T, (mp >= 0).astype(np.uint8)),
                                         rs.kf_points(sc, kf, flags), th, nnratio=0.9, check_ori=True,
                                         orb_dist=orb_dist)

    def host():
        matched = 0
        for q, (f, kfl) in enumerate(sc["queries"]):
            ransac.srand(1000 + q)
            k = sc["f_kps"][f]
            solvers = []
            for c, kf in enumerate(kfl):
                row = match[q * nc + c]
                if nmatches[q * nc + c] < reloc.MIN_MATCHES:
                    solvers.append(None)
                    continue
                idx = np.nonzero((row >= 0) & sc["valid"][kf][np.maximum(row, 0)].astype(bool))[0]
                s = ransac.PnPsolver(sc["mp_world"][kf][row[idx]], np.stack([k["x"][idx], k["y"][idx]], 1),
                                     sc["sigma2"][k["octave"][idx]], *K, indices=idx, n_matches=S)
                s.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
                solvers.append(s)
            discarded = [s is None for s in solvers]
            live, done = sum(not x for x in discarded), False
            outlier = np.zeros(S, bool)
            while live > 0 and not done:
                for c, s in enumerate(solvers):
                    if discarded[c]:
                        continue
                    T, no_more, vb, _ = s.iterate(5)
                    if no_more:
                        discarded[c] = True
                        live -= 1
                    if T is None:
                        continue
                    kf = kfl[c]
                    mp = np.where(vb, match[q * nc + c], -1)
                    found = np.zeros(S, bool)
                    found[mp[mp >= 0]] = True
                    T, n_good = optimise(f, kf, mp, T, outlier)
                    if n_good < 10:
                        continue
                    mp[outlier] = -1
                    if n_good < 50:
                        nadd, m = search(f, kf, mp, found, T, 10.0, 100)
                        mp[m >= 0] = m[m >= 0]
                        if nadd + n_good >= 50:
                            T, n_good = optimise(f, kf, mp, T, outlier)
                            if 30 < n_good < 50:
                                found[:] = False
                                found[mp[mp >= 0]] = True
                                nadd, m = search(f, kf, mp, found, T, 3.0, 64)
                                mp[m >= 0] = m[m >= 0]
                                if n_good + nadd >= 50:
                                    T, n_good = optimise(f, kf, mp, T, outlier)
                                    mp[outlier] = -1
                    if n_good >= 50:
                        matched += 1
                        done = True
                        break
        return matched

    out["host_ms"] = timed(host, max(3, a.reps // 3))
    out["host_matched"] = int(host())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
