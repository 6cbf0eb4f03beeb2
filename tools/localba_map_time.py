"""Timing of LocalBundleAdjustment from the map mirror (csrc/localba_map.hip,
csrc/localba.hip): the gather, the solve and the collection of a synthetic
neighbourhood of LocalMapping's own size -- 30 local and 20 fixed keyframes,
3,000 points, about 20,000 edges; a shape assumed, not taken from a dataset --
for one job and for 16 jobs, each with keyframes and points of its own in one
mirror.

Per case, medians over --reps rounds after --warmup, ms:
  gather    (a) orbgpu_local_ba_gather_batch_device, HIP events
  solve     (b) orbgpu_local_ba_batch_device alone on the gathered arrays, HIP events
  collect   (c) orbgpu_local_ba_collect_batch_device with the mirror written, HIP events
  chain     (d) the three on one stream, HIP events
  host_form (e) orbgpu_local_ba_batch, the host-pointer form, on the same arrays already built on the host:
            upload, solve, download -- the lower bound of the path without the mirror, whose host gather it
            leaves out entirely; host wall clock around the synchronous call
and the ratio ((a) + (c)) / (b).

    python tools/localba_map_time.py [--reps 7] [--warmup 2] [--out FILE]   # one JSON line
    python tools/localba_map_time.py --chip [--out FILE]   # the one job only: MapLocalBA.solve(chip=True)
                                     # (csrc/localba_chip.hip, the whole chip) and solve() (one workgroup) on
                                     # the same gathered arrays in the same process, alternating, and
                                     # globalba's optimize(10) on them as one problem: 3 warm-up rounds, 9
                                     # timed, a host clock around each synchronous call; FILE gets the result
                                     # under "map_time"
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "orb-slam2-annotation_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

NL, NF, M, SEE = 30, 20, 3000, 0.135


def chip_case(torch, localba, B, r, out):
    """--chip: the gathered job through the whole chip and through one workgroup, alternating, and
    globalba's optimize(10) on the same arrays (every pose past n_local fixed) for its ms per LM iteration"""
    import numpy as np

    import globalba
    B.chip_workspace()
    erase = {}
    t = {"chip": [], "one_workgroup": [], "globalba": []}
    tp, tm, te, nl = r.n_local + r.n_fixed, r.n_points, r.n_edges, r.n_local
    fixed = B.t["fixed"][:tp].clone()
    fixed[nl:] = 1
    g_T = torch.zeros((tp, 16), dtype=torch.float32, device=fixed.device)
    g_X = torch.zeros((tm, 3), dtype=torch.float32, device=fixed.device)
    g_ws = torch.empty(globalba.workspace_bytes(tp, tm, te), dtype=torch.uint8, device=fixed.device)
    g_in = [B.t[n][:{"poses": tp, "points": tm, "edges": te}[tot]] for n, _, _, tot in localba.INPUTS]
    g_in[1] = fixed

    def glob():
        return globalba.bundle_adjustment_device(*g_in, 10, 0, g_T, g_X, g_ws)

    for i in range(3 + 9):
        for name, fn in (("chip", lambda: B.solve(chip=True)), ("one_workgroup", B.solve), ("globalba", glob)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rg = fn()
            torch.cuda.synchronize()
            if i >= 3:
                t[name].append((time.perf_counter() - t0) * 1e3)
            if name != "globalba":
                erase[name] = B.t["erase"][:te].clone()
    rc = B.chip_result
    rb = B.host("results")[0]
    res = {}
    for name, its, rej in (("chip", [int(v) for v in rc["lm_iterations"]], [int(v) for v in rc["lm_rejected"]]),
                           ("one_workgroup", [int(v) for v in rb["lm_iterations"]], [int(v) for v in rb["lm_rejected"]]),
                           ("globalba", [int(rg["iterations"])], [int(rg["rejected"])])):
        ms = np.array(t[name])
        n = max(sum(its), 1)
        res[name] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                     "lm_iterations": its, "lm_rejected": rej, "ms_per_lm_iteration": float(np.median(ms)) / n,
                     "spread_ms_per_lm_iteration": float(ms.max() - ms.min()) / n}
    c, b, g = res["chip"], res["one_workgroup"], res["globalba"]
    res["chip"].update(polls=int(rc["polls"]), rounds=int(rc["rounds"]), n_erase=int(rc["n_erase"]),
                       n_free=[int(v) for v in rc["n_free"]])
    res["per_iteration_ratio"] = b["ms_per_lm_iteration"] / c["ms_per_lm_iteration"]
    res["whole_call_ratio"] = b["median_ms"] / c["median_ms"]
    res["faster_by_more_than_both_spreads"] = bool(
        b["ms_per_lm_iteration"] - c["ms_per_lm_iteration"] > c["spread_ms_per_lm_iteration"] + b["spread_ms_per_lm_iteration"])
    res["chip_over_globalba_per_iteration"] = c["ms_per_lm_iteration"] / g["ms_per_lm_iteration"]
    res["erase_equal"] = bool(torch.equal(erase["chip"], erase["one_workgroup"]))
    out.update(shape="tools/localba_map_time.py one job", n_local=nl, n_fixed=r.n_fixed, n_points=tm, n_edges=te, **res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--chip", action="store_true")
    a = ap.parse_args()
    import torch

    import localba
    import localba_map_ref as lr
    import localba_map_scene as ls
    import synth
    import track

    def events(fn, before=None):
        ts = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if before:
                before()
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return ts

    def wall(fn):
        ts = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def stat(ts):
        return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    out = {"local_kfs": NL, "fixed_kfs": NF, "points": M, "reps": a.reps, "warmup": a.warmup}
    scenes = [synth.localba_scene(NL, NF, M, 9100 + k, see=SEE, outliers=0.03) for k in range(16)]
    for name, part in (("one_job", scenes[:1]), ("batch16", scenes)):
        sc = ls.from_problems(part)
        refs = [lr.gather(sc["mirror"], sc["ba"], k, 1 << 20, 1 << 20, 1 << 20, 1 << 20) for k in sc["kfs"]]
        strides = dict(kf_stride=max(r.n_local for r in refs), pose_stride=max(r.n_local + r.n_fixed for r in refs),
                       point_stride=max(r.n_points for r in refs), edge_stride=max(r.n_edges for r in refs))
        mirror, ba = track.MapMirror(**sc["mirror"]), localba.MapMirrorBA(**sc["ba"])
        B = localba.MapLocalBA(mirror, ba, sc["kfs"], **strides)
        B.solve_workspace()
        kf_Tcw, pos = ba.t["kf_Tcw"].clone(), mirror.t["pos"].clone()

        def restore():  # the collection writes the mirror: every round starts from the same map
            ba.t["kf_Tcw"].copy_(kf_Tcw)
            mirror.t["pos"].copy_(pos)

        B.gather()
        torch.cuda.synchronize()
        G = B.host("gather_results")
        assert (G["status"] == lr.OK).all() and [int(v) for v in G["n_edges"]] == [r.n_edges for r in refs]
        if a.chip:
            out = chip_case(torch, localba, B, refs[0], out)
            break
        t_gather = events(B.gather)
        t_solve = events(B.solve)
        t_collect = events(lambda: B.collect(write_mirror=True))
        t_chain = events(lambda: B.run(write_mirror=True), before=restore)
        R = B.host("results")
        jobs, arrays = localba.make_batch([lr.problem(r) for r in refs])
        t_host = wall(lambda: localba.local_ba_batch(jobs, *(arrays[n] for n, *_ in localba.INPUTS)))
        g, s, c = (statistics.median(t) for t in (t_gather, t_solve, t_collect))
        out[name] = {"jobs": len(part), "n_local": [int(v) for v in G["n_local"]][:2], "n_fixed": [int(v) for v in G["n_fixed"]][:2],
                     "n_points": [int(v) for v in G["n_points"]][:2], "n_edges": [int(v) for v in G["n_edges"]][:2],
                     "mirror_kfs": mirror.n_kf, "mirror_points": mirror.n_pt, "rounds_min": int(R["rounds"].min()),
                     "n_erase_mean": float(B.host("n_erase").mean()), "gather_ms": stat(t_gather), "solve_ms": stat(t_solve),
                     "collect_ms": stat(t_collect), "chain_ms": stat(t_chain), "host_form_ms": stat(t_host),
                     "gather_plus_collect_over_solve": round((g + c) / s, 5)}
    line = json.dumps(out)
    print(line)
    if a.out and a.chip:
        path = Path(a.out)
        doc = json.loads(path.read_text()) if path.exists() else {}
        doc["map_time"] = out
        path.write_text(json.dumps(doc, indent=1) + "\n")
    elif a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
