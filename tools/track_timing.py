#!/usr/bin/env python3
"""Times Tracking's per-frame chain on one GPU: a batch of frames (64 x 1000
keypoints; call 1 against 1000 last-frame slots of which 300 project onto a
keypoint and 30 more are outliers, call 2 against a 2000-point local map with
250 held keypoints and 300 points to find, tests/track_scene.py) through

  new    orbgpu_track_initial_batch_device + orbgpu_track_local_map_batch_device
         enqueued back to back on one stream, one synchronise at the end,
  host   the same work driven from the host through the entries a caller had
         before: orbgpu_search_by_projection_batch_device, a readback of
         nmatches to decide the 2*th retry, a download of the rows, the gather
         on the host, an upload for orbgpu_pose_optimization_batch_device and a
         download of mvbOutlier for the cull; then orbgpu_is_in_frustum_device
         per frame, a readback of the flags for nToMatch, the LOCAL search and
         the same gather / optimise / download again.  The frame table, the
         call records and every device buffer are made before the timed region;
         inside it are the uploads, launches and readbacks the decisions need
         and the host's gather and cull in numpy (marshalled from Python, so the
         figure includes that cost).

The two halves run on two scenes of the same size (the local-map scene is not
the continuation of the first); the tables are resident in HBM before both and
their upload is not timed.  Medians of --reps calls after --warmup, a host
clock around work that ends in a device synchronise.  Prints one JSON line;
--no-host times the new calls alone (for a kernel trace).
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "orb-slam2-annotation_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--local", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    import orbgpu
    import poseopt
    import proj
    import reloc
    import track
    import track_scene as ts
    n, nk = a.frames, a.keypoints
    first = ts.initial_batch([dict(groups=[dict(n=3 * nk // 10), dict(n=3 * nk // 100, shift_px=6.0)])] * n, seed=71,
                             n_kp=nk)
    second = ts.local_batch([dict(groups=[dict(n=nk // 4, held=True), dict(n=3 * nk // 10)], n_local=a.local,
                                  n_extra=100)] * n, seed=72, n_kp=nk)
    L = orbgpu.lib()
    dev = torch.device("cuda")

    def stepper(batch):
        arrs = ts.frames_arrays(batch)
        return track.TrackStep(reloc.Frames(*arrs[:10], counts=arrs[10]))

    s1, s2 = stepper(first), stepper(second)
    tabs1 = [track.PointTable(**J["table"]) for J in first["jobs"]]
    tabs2 = [track.PointTable(**J["table"]) for J in second["jobs"]]
    s1.initial([dict(J, table=t) for J, t in zip(first["jobs"], tabs1)])
    s2.local_map([dict(J, table=t) for J, t in zip(second["jobs"], tabs2)])
    torch.cuda.synchronize()
    r1, r2 = s1.initial_results(), s2.local_results()
    out = {"frames": n, "keypoints": nk, "local_points": a.local,
           "initial_status": np.bincount([r.status for r in r1], minlength=5).tolist(),
           "initial_matches_median": int(np.median([r.nmatches for r in r1])),
           "local_status": np.bincount([r.status for r in r2], minlength=5).tolist(),
           "local_inliers_median": int(np.median([r.n_inliers for r in r2]))}

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        ts_ = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts_.append((time.perf_counter() - t0) * 1e3)
        return dict(zip(("median", "min", "max"), (statistics.median(ts_), min(ts_), max(ts_))))

    def new():
        s1.run_initial()
        s2.run_local_map()

    out["new_ms"] = timed(new, a.reps, a.warmup)
    out["new_initial_ms"] = timed(s1.run_initial, a.reps, 1)
    out["new_local_ms"] = timed(s2.run_local_map, a.reps, 1)
    if a.no_host:
        print(json.dumps(out))
        return

    # ---- the host-driven chain
    S = nk
    vp = ctypes.c_void_p

    # Outside the timed region, as a caller would hold them: the frame table on the host, one proj call
    # record per frame with everything that does not change from call to call, and every device buffer.
    def frame_table(step):
        return (reloc.RelocFrame * n).from_buffer_copy(step.frames.d_table.cpu().numpy().tobytes())

    def calls_table(ft, batch, tabs, variant, occ, extra=None):
        tab = (proj.Call * n)()
        for k, C in enumerate(tab):
            J = batch["jobs"][k]
            C.variant, C.check_ori = variant, int(variant == proj.LAST_FRAME)
            C.nnratio = 0.9 if variant == proj.LAST_FRAME else 0.8
            C.mono = int(J.get("mono", 1))
            if variant == proj.LAST_FRAME:
                C.last_Tcw[:] = [float(v) for v in np.asarray(J["last_Tcw"], np.float32).reshape(16)]
            C.target = ft[k].target
            C.target.occupied = occ.data_ptr() + k * S
            T = J["Tcw_init"] if variant == proj.LAST_FRAME else J["Tcw"]
            C.target.Tcw[:] = [float(v) for v in np.asarray(T, np.float32).reshape(16)]
            C.points = tabs[k].points(None if extra is None else J["n_local"])
            if extra is not None:
                C.points.flags, C.points.track, C.points.track_level = (e.data_ptr() + o * k for e, o in extra)
        return tab

    occ0 = torch.zeros(n * S, dtype=torch.uint8, device=dev)
    d_occ = torch.zeros((n, S), dtype=torch.uint8, device=dev)
    d_flags = torch.zeros((n, a.local), dtype=torch.int32, device=dev)
    track_buf = torch.zeros((n, a.local, 4), dtype=torch.float32, device=dev)
    level_buf = torch.zeros((n, a.local), dtype=torch.int32, device=dev)
    match = torch.zeros((n, S), dtype=torch.int32, device=dev)
    nm = torch.zeros(n, dtype=torch.int32, device=dev)
    d_calls = torch.zeros(n * ctypes.sizeof(proj.Call), dtype=torch.uint8, device=dev)
    d_jobs = torch.zeros((n, poseopt.JOB_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.zeros((n, 104), dtype=torch.uint8, device=dev)
    d_Xw = torch.zeros((n * S, 3), dtype=torch.float32, device=dev)
    d_obs = torch.zeros((n * S, 3), dtype=torch.float32, device=dev)
    d_w = torch.zeros(n * S, dtype=torch.float32, device=dev)
    d_outl = torch.zeros(n * S, dtype=torch.uint8, device=dev)
    ft1, ft2 = frame_table(s1), frame_table(s2)
    tab1 = calls_table(ft1, first, tabs1, proj.LAST_FRAME, occ0)
    tab2 = calls_table(ft2, second, tabs2, proj.LOCAL, d_occ,
                       extra=((d_flags, 4 * a.local), (track_buf, 16 * a.local), (level_buf, 4 * a.local)))
    th1 = [J["th"] for J in first["jobs"]]

    def search(tab, ths):
        """the call records with this call's th, uploaded, and the launch"""
        for C, th in zip(tab, ths):
            C.th = float(th)
        d_calls.copy_(torch.from_numpy(np.frombuffer(bytes(tab), np.uint8).copy()))
        orbgpu._check(L.orbgpu_search_by_projection_batch_device(n, vp(d_calls.data_ptr()), S, vp(match.data_ptr()),
                                                                  vp(nm.data_ptr()), None), "search")

    def optimise(batch, mps, poses, pos_of):
        """the gather on the host, the upload, PoseOptimization, the download"""
        fs = batch["frames"]
        idx = [np.nonzero(mp >= 0)[0] for mp in mps]
        Xw = np.concatenate([pos_of(k)[mps[k][i]] for k, i in enumerate(idx)]).astype(np.float32)
        obs = np.concatenate([np.stack([fs[k]["kps"]["x"][i], fs[k]["kps"]["y"][i], np.full(len(i), -1.0)], 1)
                              for k, i in enumerate(idx)]).astype(np.float32)
        w = np.concatenate([ts.INV_SIGMA2[fs[k]["kps"]["octave"][i]] for k, i in enumerate(idx)]).astype(np.float32)
        offs = np.concatenate([[0], np.cumsum([len(i) for i in idx])])
        total = len(Xw)
        jobs = poseopt.make_jobs((len(i), int(offs[k]), poses[k], ts.K, 0.0) for k, i in enumerate(idx))
        d_jobs.copy_(torch.from_numpy(jobs.view(np.uint8).reshape(n, -1)))
        d_Xw[:total].copy_(torch.from_numpy(Xw))
        d_obs[:total].copy_(torch.from_numpy(obs))
        d_w[:total].copy_(torch.from_numpy(w))
        poseopt.pose_optimization_batch_device(d_jobs, d_Xw[:total], d_obs[:total], d_w[:total], d_res, d_outl[:total])
        return idx, offs, d_res.cpu().numpy().view(poseopt.RESULT_DTYPE).reshape(n), d_outl[:total].cpu().numpy()

    host = {}

    def host_initial():
        search(tab1, th1)
        counts = nm.cpu().numpy()  # the readback the retry decision needs
        rows = match.cpu().numpy()
        if (counts < 20).any():
            search(tab1, [2 * th if c < 20 else 0.0 for th, c in zip(th1, counts)])
            again, rows2 = nm.cpu().numpy(), match.cpu().numpy()
            rows = np.where((counts < 20)[:, None], rows2, rows)
            counts = np.where(counts < 20, again, counts)
        mps = [np.where(r >= 0, r, -1) for r in rows]
        idx, offs, res, outl = optimise(first, mps, [J["Tcw_init"] for J in first["jobs"]],
                                        lambda k: first["jobs"][k]["table"]["pos"])
        nmap = []
        for k, i in enumerate(idx):  # the cull
            o = outl[offs[k]:offs[k + 1]].astype(bool)
            mps[k][i[o]] = -1
            kept = mps[k][i[~o]]
            nmap.append(int((first["jobs"][k]["table"]["flags"][kept] & 2).astype(bool).sum()))
        host["initial"] = (counts, res["n_good"].copy(), nmap)

    for k, J in enumerate(second["jobs"]):  # Frame::isInFrustum takes its pose by value from the host
        ft2[k].target.Tcw[:] = [float(v) for v in np.asarray(J["Tcw"], np.float32).reshape(16)]

    def host_local():
        mps, wflags = [], np.zeros((n, a.local), np.int32)
        for k, J in enumerate(second["jobs"]):  # :1501-1520 on the host
            fl, mp = J["table"]["flags"], J["frame_mp"].copy()
            mp[(mp >= 0) & ((fl[np.maximum(mp, 0)] & 1) == 0)] = -1
            seen = np.zeros(len(fl), bool)
            seen[mp[mp >= 0]] = True
            wflags[k] = np.where(seen[:a.local], 0, fl[:a.local] & 3)
            mps.append(mp)
        d_flags.copy_(torch.from_numpy(wflags))
        for k in range(n):
            t = tabs2[k].t
            orbgpu._check(L.orbgpu_is_in_frustum_device(
                ctypes.byref(ft2[k].target), a.local, vp(t["pos"].data_ptr()), vp(t["normal"].data_ptr()),
                vp(t["min_dist"].data_ptr()), vp(t["max_dist"].data_ptr()), ctypes.c_float(0.5),
                vp(d_flags.data_ptr() + 4 * a.local * k), vp(track_buf.data_ptr() + 16 * a.local * k),
                vp(level_buf.data_ptr() + 4 * a.local * k), None), "frustum")
        fl_back = d_flags.cpu().numpy()  # the readback nToMatch needs
        n_to_match = ((fl_back & 5) == 5).sum(1)
        occ = np.zeros((n, S), np.uint8)
        for k, J in enumerate(second["jobs"]):
            h = mps[k] >= 0
            occ[k, h] = np.where(J["table"]["flags"][mps[k][h]] & 2, 2, 1)
        d_occ.copy_(torch.from_numpy(occ))
        search(tab2, [J["th"] for J in second["jobs"]])
        rows = match.cpu().numpy()
        for k in range(n):
            if n_to_match[k] > 0:
                mps[k] = np.where(rows[k] >= 0, rows[k], mps[k])
        idx, offs, res, outl = optimise(second, mps, [J["Tcw"] for J in second["jobs"]],
                                        lambda k: second["jobs"][k]["table"]["pos"])
        inl = []
        for k, i in enumerate(idx):
            o = outl[offs[k]:offs[k + 1]].astype(bool)
            inl.append(int((second["jobs"][k]["table"]["flags"][mps[k][i[~o]]] & 2).astype(bool).sum()))
        host["local"] = (n_to_match, inl)

    def host_both():
        host_initial()
        host_local()

    out["host_ms"] = timed(host_both, max(3, a.reps // 3), a.warmup)
    # both paths did the same work
    counts, n_good, nmap = host["initial"]
    out["same_results"] = bool(
        all(max(r.nsearch) == c and r.opt.n_good == g and r.nmatches_map == m for r, c, g, m in zip(r1, counts, n_good, nmap))
        and all(r.n_to_match == t and r.n_inliers == i for r, t, i in zip(r2, *host["local"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
