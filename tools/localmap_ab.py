#!/usr/bin/env python3
"""Times an ordinary frame's chain with Tracking::UpdateLocalMap on the device
(orbgpu_update_local_map_batch_device, csrc/localmap.hip) against the path a
caller had before it, on one GPU: 64 frames of 1000 keypoints against one map
mirror of 200 keyframes x 1000 slots (15,000 points, each seen from 13
consecutive keyframes; every keyframe's covisibles are its 10 nearest in index,
its parent the one before it, its child the one after), four distinct cameras
looking at four parts of the map, each used by a quarter of the frames.  Call 1
runs against 1000 last-frame slots of which 300 project onto a keypoint and 30
more are outliers (tests/track_scene.py); those slots are points of 16
consecutive groups of the map, so 28 keyframes get votes, the K2 walk adds
eight, and the local map is about 3,400 points.

  chain    run_initial; run_update_local_map; run_local_map on one stream, one
           synchronise at the end: three calls, nothing uploaded
  parent   the previous path at its cheapest: call 1, a stream synchronise, the
           download of call 1's rows, the upload of PREBUILT tables and frame_mp
           from pinned memory (the bytes `chain` produced, made before the timed
           region), call 2, a synchronise.  The host's own UpdateLocalMap and
           table building count as zero: a lower bound for the previous path,
           not a host benchmark.

The two alternate inside one process; medians of --reps after --warmup, a host
clock around work that ends in a device synchronise.  Each call is also timed
alone.  Job 0's device result is compared with tests/localmap_ref.py, and
call 2's result bytes of the two paths with each other.  Prints one JSON line.
--chain-only runs the chain alone (for a kernel trace).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "orb-slam2-annotation_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

N_KF, GROUP, SPAN, CAMERAS = 200, 75, 13, 4


def build(n_frames, n_kp, seed=81):
    """(the call-1 batch of n_frames frames, the mirror dict, per frame src_pt_id)"""
    import track_scene as ts
    rng = np.random.default_rng(seed)
    scenes = ts.initial_batch([dict(groups=[dict(n=3 * n_kp // 10), dict(n=3 * n_kp // 100, shift_px=6.0)])] * CAMERAS,
                              seed=seed, n_kp=n_kp)
    n_pt = N_KF * GROUP
    slots = []
    for k in range(N_KF):  # keyframe k holds the groups k-12 .. k, and NULL slots up to 1000
        ids = np.arange(max(0, k - SPAN + 1) * GROUP, (k + 1) * GROUP, dtype=np.int32)
        s = np.full(1000, -1, np.int32)
        s[rng.permutation(1000)[:len(ids)]] = ids
        slots.append(s)
    obs = [[k for k in range(p // GROUP, min(p // GROUP + SPAN, N_KF))] for p in range(n_pt)]
    covis = np.full((N_KF, 10), -1, np.int32)
    for k in range(N_KF):
        near = [k + d * s for d in range(1, 6) for s in (1, -1)]
        near = [c for c in near if 0 <= c < N_KF]
        covis[k, :len(near)] = near
    kf_bad = np.zeros(N_KF, np.uint8)
    kf_bad[rng.choice(N_KF, 3, replace=False)] = 1
    pt_flags = np.where(rng.random(n_pt) < 0.98, 3, 2).astype(np.int32)
    pos = rng.uniform(-20, 20, (n_pt, 3)).astype(np.float32)
    desc = rng.integers(0, 256, (n_pt, 32), dtype=np.uint8)
    octave = rng.integers(0, 4, n_pt)
    centre = np.zeros((n_pt, 3))
    srcs = []
    for q in range(CAMERAS):
        f, tab = scenes["frames"][q], scenes["jobs"][q]["table"]
        lo = (50 * q - 8) * GROUP
        near = np.arange(max(lo, 0), (50 * q + 50) * GROUP)  # what this camera's local map can reach
        pos[near] = ts.random_world(f, rng, len(near))
        centre[near] = f["C"]
        mine = np.arange((50 * q + 12) * GROUP, (50 * q + 28) * GROUP)
        src = rng.permutation(mine)[:n_kp].astype(np.int32)  # call 1's slot t is the map's point src[t]
        held = (tab["flags"] & 1) != 0  # a NULL slot names nothing
        pos[src[held]], desc[src[held]], octave[src[held]] = tab["pos"][held], tab["desc"][held], tab["octave"][held]
        pt_flags[src[held]] = 3
        srcs.append(np.where(held, src, -1).astype(np.int32))
    d = pos.astype(np.float64) - centre
    dist = np.maximum(np.linalg.norm(d, axis=1), 1e-6)
    max_dist = (dist * ts.SF[octave] * 0.95).astype(np.float32)
    mirror = {"kf_bad": kf_bad, "slots": slots, "covis": covis, "children": [[k + 1] if k + 1 < N_KF else [] for k in range(N_KF)],
              "parent": np.arange(-1, N_KF - 1, dtype=np.int32), "kf_by_rank": None, "pt_flags": pt_flags, "obs": obs,
              "pos": pos, "normal": (d / dist[:, None]).astype(np.float32), "desc": desc,
              "min_dist": (max_dist / ts.SF[7]).astype(np.float32), "max_dist": max_dist}
    batch = {"stereo": False, "frames": [scenes["frames"][k % CAMERAS] for k in range(n_frames)],
             "jobs": [dict(scenes["jobs"][k % CAMERAS], frame=k) for k in range(n_frames)]}
    return batch, mirror, [srcs[k % CAMERAS] for k in range(n_frames)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--point-stride", type=int, default=6144)
    ap.add_argument("--kf-stride", type=int, default=96)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain-only", action="store_true")
    a = ap.parse_args()
    batch, mirror, srcs = build(a.frames, a.keypoints)
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    import localmap_ref as lr
    import reloc
    import track
    import track_scene as ts
    n, P = a.frames, a.point_stride
    arrs = ts.frames_arrays(batch)
    step = track.TrackStep(reloc.Frames(*arrs[:10], counts=arrs[10]))
    tabs = [track.PointTable(**batch["jobs"][q]["table"]) for q in range(CAMERAS)]
    step.initial([dict(J, table=tabs[k % CAMERAS]) for k, J in enumerate(batch["jobs"])])
    d_mirror = track.MapMirror(**mirror)
    while True:  # the second time with the point_stride a caller who knows the map's size would choose
        step.prepare_local_map([dict(frame=k, Tcw=step.initial_pose_ptr(k), th=1.0) for k in range(n)], P)
        step.update_local_map([dict(n_kp=a.keypoints, src_pt_id=srcs[k], table=tabs[k % CAMERAS], prev_kfs=[])
                               for k in range(n)], d_mirror, kf_stride=a.kf_stride)
        step.run_local_map()
        torch.cuda.synchronize()
        r1, ru, r2 = step.initial_results(), step.update_results(), step.local_results()
        fit = -(-max(r.n_local + r.n_extra for r in ru) // 64) * 64
        if fit >= P:
            break
        P = fit
    rows0 = step.initial_rows()[0]
    want = lr.update_local_map(mirror, dict(n_kp=a.keypoints, rows=rows0, src_pt_id=srcs[0],
                                            src_pos=batch["jobs"][0]["table"]["pos"],
                                            src_desc=batch["jobs"][0]["table"]["desc"], prev_kfs=[]), step.stride, P,
                               a.kf_stride)
    tables = step.prepared_tables()
    same = (ru[0].status, ru[0].n_k1, ru[0].n_local_kfs, ru[0].ref_kf, ru[0].n_nulled, ru[0].n_local, ru[0].n_extra) == \
        (want.status, want.n_k1, want.n_local_kfs, want.ref_kf, want.n_nulled, want.n_local, want.n_extra) and \
        step.local_kfs()[0][:want.n_local_kfs].tolist() == want.local_kfs and \
        step.local_points()[0][:want.n_local].tolist() == want.local_points and \
        np.array_equal(step.prepared_frame_mp()[0][:a.keypoints], want.frame_mp) and \
        all(tables[name][0][:want.points_n].tobytes() == np.ascontiguousarray(want.table[name]).tobytes() for name in tables)
    out = {"frames": n, "keypoints": a.keypoints, "mirror_keyframes": N_KF, "mirror_points": N_KF * GROUP,
           "initial_status": np.bincount([r.status for r in r1], minlength=5).tolist(),
           "update_status": np.bincount([r.status for r in ru], minlength=4).tolist(),
           "local_status": np.bincount([r.status for r in r2], minlength=5).tolist(),
           "k1_median": int(np.median([r.n_k1 for r in ru])),
           "local_kfs_median": int(np.median([r.n_local_kfs for r in ru])),
           "local_points_median": int(np.median([r.n_local for r in ru])),
           "extras_median": int(np.median([r.n_extra for r in ru])),
           "n_to_match_median": int(np.median([r.n_to_match for r in r2])),
           "local_inliers_median": int(np.median([r.n_inliers for r in r2])),
           "job0_equals_reference": bool(same),
           "point_stride": P, "workspace_mb": round(step.lm_ws.numel() / 2 ** 20, 1)}
    chain_bytes = bytes(step.d_local_results.cpu().numpy())
    stream = torch.cuda.Stream()

    def chain():
        step.run_initial(stream)
        step.run_update_local_map(stream)
        step.run_local_map(stream)
        stream.synchronize()

    # the parent's path: the tables the host would have built, in pinned memory before the clock starts
    pinned = {name: t.cpu().pin_memory() for name, t in step.d_table.items()}
    pinned_mp = step.d_frame_mp.cpu().pin_memory()
    rows_host = torch.empty(step.d_initial_rows.shape, dtype=torch.int32).pin_memory()
    upload_mb = (sum(t.numel() * t.element_size() for t in pinned.values()) + pinned_mp.numel() * 4) / 2 ** 20

    def parent():
        step.run_initial(stream)
        with torch.cuda.stream(stream):
            rows_host.copy_(step.d_initial_rows, non_blocking=True)
        stream.synchronize()  # the host reads the rows here
        with torch.cuda.stream(stream):
            for name, t in step.d_table.items():
                t.copy_(pinned[name], non_blocking=True)
            step.d_frame_mp.copy_(pinned_mp, non_blocking=True)
        step.run_local_map(stream)
        stream.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts_):
        return {"median": round(statistics.median(ts_), 4), "min": round(min(ts_), 4), "max": round(max(ts_), 4)}

    if a.chain_only:
        for _ in range(a.warmup + a.reps):
            chain()
        print(json.dumps(out))
        return
    for _ in range(a.warmup):
        chain()
        parent()
    tc, tp = [], []
    for _ in range(a.reps):  # alternating, so that both see the same machine
        tc.append(clock(chain))
        tp.append(clock(parent))
    out["chain_ms"], out["parent_lower_bound_ms"] = stats(tc), stats(tp)
    out["parent_upload_mb"] = round(upload_mb, 1)
    out["parent_equals_chain"] = bytes(step.d_local_results.cpu().numpy()) == chain_bytes
    for name, fn in (("initial_ms", step.run_initial), ("update_local_map_ms", step.run_update_local_map),
                     ("local_map_ms", step.run_local_map)):
        out[name] = stats([clock(lambda: fn(stream)) for _ in range(a.reps)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
