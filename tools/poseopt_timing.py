"""Motion-only pose optimisation on one MI355X (csrc/poseopt.hip).

Device form: `--batch` jobs of n = 300 and of n = 1000 observations (20 %
gross outliers, half of the edges stereo, start 0.03 rad / 5 cm off), one
launch per call: median / min / max of event-timed calls, the LM iterations
the jobs ran (sum over the four rounds, mean over the jobs) and the kernel
time over that mean -- the time per LM iteration of a job while the whole
batch is in flight.  Host form: one n = 300 job, upload + launch + download +
synchronise, wall clock around the synchronous call.

The workgroup size is fixed when the library is built (POSEOPT_THREADS in
csrc/poseopt.hip, 256).  For the A/B, build variant libraries beside the
product one and name them with --variant; each library is timed by a child
process of its own (ORBGPU_LIBRARY selects it), the product library first:

  make -C orb-slam2-annotation_amd BUILD=build_t64 LIB=liborbgpu_t64.so EXTRA=-DPOSEOPT_THREADS=64
  make -C orb-slam2-annotation_amd BUILD=build_t128 LIB=liborbgpu_t128.so EXTRA=-DPOSEOPT_THREADS=128
  python tools/poseopt_timing.py --variant 64=orb-slam2-annotation_amd/liborbgpu_t64.so \
                                 --variant 128=orb-slam2-annotation_amd/liborbgpu_t128.so

No CPU figure is given: g2o cannot be built here.  Prints one JSON document
and writes it to --out.

usage: python tools/poseopt_timing.py [--batch 512] [--calls 30] [--warmup 5] [--variant THREADS=LIB ...]
                                      [--out profiles/poseopt_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "orb-slam2-annotation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbgpu  # noqa: E402
import poseopt  # noqa: E402
import synth  # noqa: E402


def timed(fn, calls, warmup):
    """median / min / max milliseconds of `calls` event-timed calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return statistics.median(ms), min(ms), max(ms)


def batch_of(B, n, seed0):
    scenes = [synth.pose_scene(n, seed0 + k, outliers=0.2, stereo=0.5) for k in range(B)]
    jobs = poseopt.make_jobs([(n, k * n, s["Tcw0"], s["K"], s["bf"]) for k, s in enumerate(scenes)])
    cat = lambda key: np.concatenate([s[key].reshape(n, -1) for s in scenes])
    return jobs, cat("Xw"), cat("obs"), cat("inv_sigma2").reshape(-1)


def measure(a, threads):
    """the result records of the library this process has loaded"""
    B = a.batch
    results = []
    for n in (300, 1000):
        jobs, Xw, obs, w = batch_of(B, n, 10_000 * n)
        d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(B, -1)).cuda()
        d_X, d_o, d_w = (torch.from_numpy(v).cuda() for v in (Xw, obs, w))
        d_res = torch.zeros((B, poseopt.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(B * n, dtype=torch.uint8, device="cuda")
        med, lo, hi = timed(lambda: poseopt.pose_optimization_batch_device(d_jobs, d_X, d_o, d_w, d_res, d_out),
                            a.calls, a.warmup)
        res = d_res.cpu().numpy().reshape(-1).view(poseopt.RESULT_DTYPE)
        its = res["lm_iterations"].sum(1)
        results.append({"case": f"device_form_b{B}_n{n}", "threads": threads, "ms_median": round(med, 4),
                        "ms_min": round(lo, 4), "ms_max": round(hi, 4), "us_per_job": round(med * 1e3 / B, 3),
                        "lm_iterations_per_job_mean": round(float(its.mean()), 2),
                        "lm_rejected_per_job_mean": round(float(res["lm_rejected"].sum(1).mean()), 2),
                        "us_per_lm_iteration": round(med * 1e3 / float(its.mean()), 3),
                        "n_good_sum": int(res["n_good"].sum())})
    # host form, one job
    jobs, Xw, obs, w = batch_of(1, 300, 77)
    out = np.zeros(300, np.uint8)
    for _ in range(a.warmup):
        poseopt.pose_optimization_batch(jobs, Xw, obs, w, out)
    us = []
    for _ in range(max(a.calls, 50)):
        t0 = time.perf_counter()
        poseopt.pose_optimization_batch(jobs, Xw, obs, w, out)
        us.append((time.perf_counter() - t0) * 1e6)
    res, _ = poseopt.pose_optimization_batch(jobs, Xw, obs, w, out)
    results.append({"case": "host_form_1_job_n300", "threads": threads, "us_median": round(statistics.median(us), 2),
                    "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                    "lm_iterations": int(res["lm_iterations"].sum()), "lm_rejected": int(res["lm_rejected"].sum()),
                    "timing": "wall clock around the synchronous call, ctypes wrapper included"})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variant", action="append", default=[], metavar="THREADS=LIB",
                    help="a library built with -DPOSEOPT_THREADS=THREADS, timed in a child process")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "poseopt_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "poseopt_timing needs a GPU"
    assert a.calls >= 20, "the median is taken over at least 20 timed calls"
    if a.child is not None:  # one library, results on the last line of stdout
        print(json.dumps(measure(a, a.child)))
        return
    results = measure(a, 256)
    for v in a.variant:
        threads, lib = v.split("=", 1)
        env = dict(os.environ, ORBGPU_LIBRARY=str(Path(lib).resolve()))
        r = subprocess.run([sys.executable, __file__, "--child", threads, "--batch", str(a.batch), "--calls",
                            str(a.calls), "--warmup", str(a.warmup)], env=env, check=True, capture_output=True,
                           text=True, timeout=600)
        results += json.loads(r.stdout.strip().split("\n")[-1])
    doc = {"tool": "tools/poseopt_timing.py", "device": orbgpu.device_arch(),
           "timing": f"device form: median of {a.calls} event-timed calls after {a.warmup} warm-up calls, one launch "
                     "per call; 20 % outliers, half of the edges stereo; threads = the library's workgroup size "
                     "(256: the product library, others: variant builds, one process each)",
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text + "\n")


if __name__ == "__main__":
    main()
