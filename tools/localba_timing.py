"""Timing of the local bundle adjustment (csrc/localba.hip): one job and 64 jobs
of 20 free poses, 10 fixed poses, 2,000 points and about 12,000 monocular
edges -- a shape assumed for LocalMapping's neighbourhoods, not taken from a
dataset -- device-resident inputs, ms per call from HIP events, with the LM
iteration and rejected-trial counts of the jobs (a pass over the edges per
iteration and per trial).  One job runs on one workgroup, that is on one CU of
the chip; the 64-job call fills 64 of them.

    python tools/localba_timing.py            # the timings, one JSON line
    python tools/localba_timing.py --profile [--out DIR]  # the same under rocprofv3 --kernel-trace
                                              # --stats, in a child process; output under DIR
                                              # (default bench_out/localba_prof)
    python tools/localba_timing.py --chip [--out FILE]  # the one job through orbgpu_local_ba_chip_device
                                              # (csrc/localba_chip.hip, the whole chip) and through the
                                              # one-workgroup call on the same arrays in the same process,
                                              # alternating: 3 warm-up rounds, 9 timed, a host clock around
                                              # each synchronous call; FILE gets the result under "timing"
"""
import json
import subprocess
import sys

sys.path.insert(0, "orb-slam2-annotation_amd")
sys.path.insert(0, "oracle")

if "--profile" in sys.argv:
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "bench_out/localba_prof"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--", sys.executable, __file__, "--reps", "1"]
    sys.exit(subprocess.run(cmd, timeout=900).returncode)

import numpy as np
import torch

import localba
import synth

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
dev = torch.device("cuda:0")
NL, NF, M, BATCH = 20, 10, 2000, 64


def chip_against_one_workgroup(chip, batch, warmup=3, rounds=9):
    """the two synchronous calls alternating; chip() returns its CHIP_RESULT_DTYPE record, batch() the
    (iterations, rejected) of the one-workgroup job.  Medians with min and max, and ms per LM iteration"""
    import time
    t = {"chip": [], "one_workgroup": []}
    for i in range(warmup + rounds):
        for name, fn in (("chip", chip), ("one_workgroup", batch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if i >= warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
            if name == "chip":
                rc = r
            else:
                rb = r
    out = {}
    for name, its, rej in (("chip", [int(v) for v in rc["lm_iterations"]], [int(v) for v in rc["lm_rejected"]]),
                           ("one_workgroup", rb[0], rb[1])):
        ms = np.array(t[name])
        n = max(sum(its), 1)
        out[name] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                     "lm_iterations": its, "lm_rejected": rej, "ms_per_lm_iteration": float(np.median(ms)) / n,
                     "spread_ms_per_lm_iteration": float(ms.max() - ms.min()) / n}
    out["chip"].update(polls=int(rc["polls"]), rounds=int(rc["rounds"]), n_erase=int(rc["n_erase"]),
                       n_free=[int(v) for v in rc["n_free"]])
    a, b = out["chip"], out["one_workgroup"]
    out["per_iteration_ratio"] = b["ms_per_lm_iteration"] / a["ms_per_lm_iteration"]
    out["whole_call_ratio"] = b["median_ms"] / a["median_ms"]
    out["faster_by_more_than_both_spreads"] = bool(
        b["ms_per_lm_iteration"] - a["ms_per_lm_iteration"] > a["spread_ms_per_lm_iteration"] + b["spread_ms_per_lm_iteration"])
    return out


if "--chip" in sys.argv:
    s = synth.localba_scene(NL, NF, M, 9000, see=0.2, outliers=0.03)
    jobs, a = localba.make_batch([s])
    tp, tm, te = len(a["Tcw"]), len(a["Xw"]), len(a["obs"])
    d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(1, -1)).to(dev)
    d_in = [torch.from_numpy(np.ascontiguousarray(a[n])).to(dev) for n, *_ in localba.INPUTS]
    outs = [[torch.zeros((NL, 16), dtype=torch.float32, device=dev), torch.zeros((tm, 3), dtype=torch.float32, device=dev),
             torch.zeros(te, dtype=torch.uint8, device=dev)] for _ in range(2)]
    d_res = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    d_ws = torch.empty(localba.workspace_bytes(1, tp, tm, te, NL), dtype=torch.uint8, device=dev)
    c_ws = torch.empty(localba.chip_workspace_bytes(tp, NL, tm, te), dtype=torch.uint8, device=dev)

    def batch():
        localba.local_ba_batch_device(d_jobs, *d_in, *outs[1], d_res, d_ws, NL)
        torch.cuda.synchronize()
        r = d_res.cpu().numpy().reshape(-1).view(localba.RESULT_DTYPE)[0]
        return [int(v) for v in r["lm_iterations"]], [int(v) for v in r["lm_rejected"]]

    res = {"shape": "tools/localba_timing.py one job", "free_poses": NL, "fixed_poses": NF, "points": M, "edges": te,
           "chip_workspace_MiB": c_ws.numel() / 2 ** 20}
    res.update(chip_against_one_workgroup(lambda: localba.local_ba_chip_device(*d_in, NL, *outs[0], c_ws), batch))
    res["erase_equal"] = bool(torch.equal(outs[0][2], outs[1][2]))
    res["max_abs_pose_difference"] = float((outs[0][0] - outs[1][0]).abs().max())
    print(json.dumps(res))
    if "--out" in sys.argv:
        from pathlib import Path
        path = Path(sys.argv[sys.argv.index("--out") + 1])
        doc = json.loads(path.read_text()) if path.exists() else {}
        doc["timing"] = res
        path.write_text(json.dumps(doc, indent=1) + "\n")
    sys.exit(0)

scenes = [synth.localba_scene(NL, NF, M, 9000 + k, see=0.2, outliers=0.03) for k in range(BATCH)]
res = {"free_poses": NL, "fixed_poses": NF, "points": M, "edges_job0": int(len(scenes[0]["obs"]))}
for name, part in (("one_job", scenes[:1]), ("batch64", scenes)):
    jobs, a = localba.make_batch(part)
    B, tp, tm, te = len(jobs), len(a["Tcw"]), len(a["Xw"]), len(a["obs"])
    d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(B, -1)).to(dev)
    d_in = [torch.from_numpy(np.ascontiguousarray(a[n])).to(dev) for n, *_ in localba.INPUTS]
    d_T = torch.zeros((B * NL, 16), dtype=torch.float32, device=dev)
    d_X = torch.zeros((tm, 3), dtype=torch.float32, device=dev)
    d_e = torch.zeros(te, dtype=torch.uint8, device=dev)
    d_res = torch.zeros((B, 32), dtype=torch.uint8, device=dev)
    ws_bytes = localba.workspace_bytes(B, tp, tm, te, NL)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call():
        localba.local_ba_batch_device(d_jobs, *d_in, d_T, d_X, d_e, d_res, d_ws, NL)

    call()  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    r = d_res.cpu().numpy().reshape(-1).view(localba.RESULT_DTYPE)
    it, rej = r["lm_iterations"].astype(int), r["lm_rejected"].astype(int)
    res[name] = {"ms_per_call": e0.elapsed_time(e1) / reps, "jobs": B, "edges": te, "workspace_MiB": ws_bytes / 2 ** 20,
                 "rounds_min": int(r["rounds"].min()), "n_erase_mean": float(r["n_erase"].mean()),
                 "iterations_mean": [float(v) for v in it.mean(0)], "rejected_mean": [float(v) for v in rej.mean(0)],
                 # a build pass per iteration, a trial pass per trial: at most one accepted trial per iteration
                 "edge_passes_upper_mean": float((2 * it.sum(1) + rej.sum(1)).mean())}
print(json.dumps(res))
