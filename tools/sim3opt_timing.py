"""Sim3 refinement (Optimizer::OptimizeSim3) on one MI355X (csrc/sim3opt.hip).

Device form: batches of 1, 64 and 512 jobs of n = 100 and of n = 300
correspondences (20 % gross outliers, start 0.02 rad / 5 cm / 3 % in scale
off), one launch per call: median / min / max of event-timed calls in
microseconds per batch, the LM iterations and rejected trials the jobs ran
(sum over the two optimisations, mean over the jobs).  Host form: one n = 100
job, upload + launch + download + synchronise, wall clock around the
synchronous call.

No CPU figure is given: g2o cannot be built here.  Prints one JSON document
and writes it to --out.

usage: python tools/sim3opt_timing.py [--calls 30] [--warmup 5] [--out profiles/sim3opt_timing.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "orb-slam2-annotation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbgpu  # noqa: E402
import sim3opt  # noqa: E402
import synth  # noqa: E402


def timed(fn, calls, warmup):
    """median / min / max microseconds of `calls` event-timed calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in evs]
    return statistics.median(us), min(us), max(us)


def batch_of(B, n, seed0, pool=64):
    """B jobs over at most `pool` distinct scenes (each job has its own copy of the correspondences)"""
    scenes = [synth.sim3opt_scene(n, seed0 + k, fix_scale=k % 2 == 1) for k in range(min(B, pool))]
    scenes = [scenes[k % len(scenes)] for k in range(B)]
    jobs = sim3opt.make_jobs([(n, k * n, s["q12"], s["t12"], s["s12"], s["K1"], s["K2"], s["th2"], s["fix_scale"])
                              for k, s in enumerate(scenes)])
    arrays = [np.concatenate([s[key].reshape(n, w) for s in scenes]) for key, w in sim3opt.ARRAYS]
    arrays[4], arrays[5] = arrays[4].reshape(-1), arrays[5].reshape(-1)
    return jobs, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sim3opt_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sim3opt_timing needs a GPU"
    assert a.calls >= 20, "the median is taken over at least 20 timed calls"
    results = []
    for n in (100, 300):
        for B in (1, 64, 512):
            jobs, arrays = batch_of(B, n, 10_000 * n)
            d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(B, -1)).cuda()
            d_arrays = [torch.from_numpy(v).cuda() for v in arrays]
            d_res = torch.zeros((B, sim3opt.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(B * n, dtype=torch.uint8, device="cuda")
            med, lo, hi = timed(lambda: sim3opt.optimize_sim3_batch_device(d_jobs, *d_arrays, d_res, d_out),
                                a.calls, a.warmup)
            res = d_res.cpu().numpy().reshape(-1).view(sim3opt.RESULT_DTYPE)
            results.append({"case": f"device_form_b{B}_n{n}", "us_median": round(med, 2), "us_min": round(lo, 2),
                            "us_max": round(hi, 2), "us_per_job": round(med / B, 3),
                            "lm_iterations_per_job_mean": round(float(res["lm_iterations"].sum(1).mean()), 2),
                            "lm_rejected_per_job_mean": round(float(res["lm_rejected"].sum(1).mean()), 2),
                            "rounds_2": int((res["rounds"] == 2).sum()), "n_in_sum": int(res["n_in"].sum())})
    # host form, one job
    jobs, arrays = batch_of(1, 100, 77)
    out = np.zeros(100, np.uint8)
    for _ in range(a.warmup):
        sim3opt.optimize_sim3_batch(jobs, *arrays, out)
    us = []
    for _ in range(max(a.calls, 50)):
        t0 = time.perf_counter()
        sim3opt.optimize_sim3_batch(jobs, *arrays, out)
        us.append((time.perf_counter() - t0) * 1e6)
    res, _ = sim3opt.optimize_sim3_batch(jobs, *arrays, out)
    results.append({"case": "host_form_1_job_n100", "us_median": round(statistics.median(us), 2),
                    "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                    "lm_iterations": int(res["lm_iterations"].sum()), "lm_rejected": int(res["lm_rejected"].sum()),
                    "timing": "wall clock around the synchronous call, ctypes wrapper included"})
    doc = {"tool": "tools/sim3opt_timing.py", "device": orbgpu.device_arch(),
           "timing": f"device form: median of {a.calls} event-timed calls after {a.warmup} warm-up calls, one launch "
                     "per call; 20 % outliers, every other job with fix_scale; 256 threads per job",
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text + "\n")


if __name__ == "__main__":
    main()
