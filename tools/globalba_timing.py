"""Timing of the global bundle adjustment (csrc/globalba.hip) on three shapes,
each assumed, not taken from a dataset:

  (i)   the monocular initial map: 2 keyframes, 150 points, 20 iterations, robust;
  (ii)  the LocalBA shape of tools/localba_timing.py as one problem: 30 poses with
        pose 0 fixed, 2,000 points, about 12,200 monocular edges, 10 iterations,
        robust -- and orbgpu_local_ba_batch_device (one workgroup) on the same
        arrays in the same process, the two calls alternating;
  (iii) a loop-closure map: 300 keyframes, 30,000 points, about 150,000 edges, 10
        iterations, not robust.

Device-resident inputs, a host clock around the synchronous call (the LocalBA call
is followed by a stream synchronisation), 3 warm-up rounds and 9 timed ones:
median, minimum and maximum in ms, the LM iterations and rejected trials, ms per
LM iteration, and the launches and synchronisations of one trial.

    python tools/globalba_timing.py            # the timings, one JSON line
    python tools/globalba_timing.py --shapes ii,iii        # some of the shapes only
    python tools/globalba_timing.py --profile [--shapes iii] [--out DIR]  # one round of the shapes under
                                               # rocprofv3 --kernel-trace --stats (CSV), in a child process;
                                               # output under DIR (default bench_out/globalba_prof)
"""
import json
import subprocess
import sys
import time

sys.path.insert(0, "orb-slam2-annotation_amd")
sys.path.insert(0, "oracle")

if "--profile" in sys.argv:
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "bench_out/globalba_prof"
    shapes = sys.argv[sys.argv.index("--shapes") + 1] if "--shapes" in sys.argv else "i,ii,iii"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "globalba", "--",
           sys.executable, __file__, "--warmup", "0", "--rounds", "1", "--shapes", shapes]
    sys.exit(subprocess.run(cmd, timeout=900).returncode)

import numpy as np
import torch

import globalba
import localba
import synth

WARMUP = int(sys.argv[sys.argv.index("--warmup") + 1]) if "--warmup" in sys.argv else 3
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 9
SHAPES = (sys.argv[sys.argv.index("--shapes") + 1] if "--shapes" in sys.argv else "i,ii,iii").split(",")
NB = 48  # csrc/globalba.hip: kNB
dev = torch.device("cuda:0")


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def launches_per_trial(n_free):
    """point inverse, B Dinv, Schur; per panel diagonal block, panel rows, trailing update (none after the
    last); per panel of the back-substitution its block and the rows above (none above the first); x_l,
    trial, chi2 pass, judge -- and the copy of an accepted trial.  One synchronisation per trial."""
    panels = -(-6 * n_free // NB)
    return 2 + (1 + 3 * panels - 1 + 2 * panels - 1 if n_free else 0) + 4 + 1


def upload(s):
    a = globalba.pack(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"], s["obs"], s["inv_sigma2"])
    return a, [torch.from_numpy(a[n]).to(dev) for n, *_ in globalba.INPUTS]


def global_call(s, n_iterations, robust):
    a, d_in = upload(s)
    tp, tm, te = len(a["Tcw"]), len(a["Xw"]), len(a["obs"])
    d_T = torch.zeros((tp, 16), dtype=torch.float32, device=dev)
    d_X = torch.zeros((tm, 3), dtype=torch.float32, device=dev)
    ws_bytes = globalba.workspace_bytes(tp, tm, te)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    box = {}

    def call():
        box["res"] = globalba.bundle_adjustment_device(*d_in, n_iterations, robust, d_T, d_X, d_ws)

    return call, box, {"poses": tp, "points": tm, "edges": te, "workspace_MiB": ws_bytes / 2 ** 20}


def local_call(s):
    jobs, a = localba.make_batch([s])
    tp, tm, te, NL = len(a["Tcw"]), len(a["Xw"]), len(a["obs"]), int(s["n_local"])
    d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(1, -1)).to(dev)
    d_in = [torch.from_numpy(np.ascontiguousarray(a[n])).to(dev) for n, *_ in localba.INPUTS]
    d_T = torch.zeros((NL, 16), dtype=torch.float32, device=dev)
    d_X = torch.zeros((tm, 3), dtype=torch.float32, device=dev)
    d_e = torch.zeros(te, dtype=torch.uint8, device=dev)
    d_res = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    d_ws = torch.empty(localba.workspace_bytes(1, tp, tm, te, NL), dtype=torch.uint8, device=dev)

    def call():
        localba.local_ba_batch_device(d_jobs, *d_in, d_T, d_X, d_e, d_res, d_ws, NL)
        torch.cuda.synchronize()

    return call, lambda: d_res.cpu().numpy().reshape(-1).view(localba.RESULT_DTYPE)[0]


def timed(calls):
    """every call of `calls` in turn, WARMUP + ROUNDS times; ms per call of the timed rounds"""
    ms = [[] for _ in calls]
    for rnd in range(WARMUP + ROUNDS):
        for k, call in enumerate(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if rnd >= WARMUP:
                ms[k].append(1e3 * (t1 - t0))
    return ms


def report(box, shape, ms):
    r = box["res"]
    it = int(r["iterations"])
    out = dict(shape, **stats(ms), iterations=it, rejected=int(r["rejected"]), n_free=int(r["n_free"]),
               first_chi2=float(r["first_chi2"]), last_chi2=float(r["last_chi2"]),
               launches_per_trial=launches_per_trial(int(r["n_free"])), synchronisations_per_trial=1)
    out["ms_per_iteration"] = {k: v / max(it, 1) for k, v in stats(ms).items()}
    return out


res = {"warmup_rounds": WARMUP, "timed_rounds": ROUNDS}

if "i" in SHAPES:
    s = synth.localba_scene(2, 0, 150, 2501, kf0_local=True)
    call, box, shape = global_call(s, 20, 1)
    res["initial_map"] = report(box, shape, timed([call])[0])

if "ii" in SHAPES:
    s = synth.localba_scene(30, 0, 2000, 9000, see=0.2, outliers=0.03, kf0_local=True)
    call, box, shape = global_call(s, 10, 1)
    lcall, lres = local_call(s)
    ms_g, ms_l = timed([call, lcall])
    res["localba_shape"] = report(box, shape, ms_g)
    lr = lres()
    lit = int(lr["lm_iterations"].sum())
    res["localba_shape"]["local_ba_one_workgroup"] = dict(stats(ms_l), lm_iterations=[int(v) for v in lr["lm_iterations"]],
                                                          lm_rejected=[int(v) for v in lr["lm_rejected"]],
                                                          ms_per_iteration={k: v / max(lit, 1) for k, v in stats(ms_l).items()})
    g, l = res["localba_shape"]["ms_per_iteration"], res["localba_shape"]["local_ba_one_workgroup"]["ms_per_iteration"]
    spreads = (g["max_ms"] - g["min_ms"]) + (l["max_ms"] - l["min_ms"])
    res["localba_shape"]["per_iteration_gain_ms"] = l["median_ms"] - g["median_ms"]
    res["localba_shape"]["both_spreads_ms"] = spreads
    res["localba_shape"]["faster_by_more_than_both_spreads"] = bool(l["median_ms"] - g["median_ms"] > spreads)

if "iii" in SHAPES:
    s = synth.localba_scene(300, 0, 30000, 9100, see=5.0 / 300, kf0_local=True)
    call, box, shape = global_call(s, 10, 0)
    res["loop_closure_map"] = report(box, shape, timed([call])[0])
print(json.dumps(res))
