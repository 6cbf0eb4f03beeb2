"""Timing of KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling on the covisibility table
(csrc/covis.hip): a camera that goes four times round a ring of 500 places, 2,000 keyframes, 40,000 points; the
table is filled on the device by UpdateConnections of every keyframe.

  update_1 / update_64   orbgpu_covis_update_connections_batch_device for the last keyframe and for the last 64:
                         those keyframes are first erased from the table (SetBadFlag's erasure), so every
                         AddConnection is an insertion and a rebuild, as for keyframes that are new; the table is
                         restored before each call, outside the timed span
  culling                orbgpu_covis_keyframe_culling_batch_device, one stereo job for the last keyframe

Device events around the library call on buffers allocated beforehand, the median of 20 calls after 3 warm-up
calls, min-max beside it.

    python tools/covis_timing.py [--out FILE]      # one JSON line, and the row for DESIGN section 10
    python tools/covis_timing.py --apply FILE      # no GPU: writes the row of FILE into DESIGN.md
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "orb-slam2-annotation_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

N_KF, LOOPS, PTS, STRIDE, SEED = 2000, 4, 80, 512, 5
WARMUP, REPS = 3, 20
HEAD = "**Covisibility graph: UpdateConnections and KeyFrameCulling**"


def row(r):
    f = lambda t: f"**{t['median']:.3f} ms** ({t['min']:.3f}–{t['max']:.3f})"
    return (f"{HEAD} (§5s; `tools/covis_timing.py`; a looping path of {r['n_kf']:,} keyframes and {r['n_pt']:,} points, "
            f"{r['slots_per_kf']:.0f} slots per keyframe and {r['obs_per_pt']:.1f} observations per point on average, "
            f"the table filled on the device, rows of {r['conn_stride']}; device events around the call, median of {REPS} "
            f"after {WARMUP} warm-up calls, min–max in brackets): `orbgpu_covis_update_connections_batch_device` for one new "
            f"keyframe {f(r['update_1'])} ({r['update_1_counted']} counted, {r['update_1_ordered']} of them from 15 on), for 64 "
            f"new keyframes in one call {f(r['update_64'])}; `orbgpu_covis_keyframe_culling_batch_device`, one stereo job "
            f"with a list of {r['cull_list']} of which {r['cull_culled']} are culled, {f(r['culling'])}. These are first "
            f"numbers: there is no earlier device path to compare them with and no threshold was set for them.")


def apply(path):
    r = json.loads(Path(path).read_text().splitlines()[0])
    design = ROOT / "DESIGN.md"
    lines = design.read_text().split("\n")
    lines = [ln for ln in lines if not ln.startswith(HEAD)]
    at = lines.index("## 11. Out of scope")
    while lines[at - 1] == "" and lines[at - 2] == "":
        del lines[at - 1]
        at -= 1
    lines[at:at] = [row(r), ""]
    design.write_text("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--apply", default=None)
    a = ap.parse_args()
    if a.apply:
        return apply(a.apply)
    import numpy as np
    import torch

    import covis
    import covis_update_ref as cur
    import orbgpu
    from test_covis_update import to_device

    S = cur.Scene(N_KF)
    S.first[0] = 1
    rng = np.random.default_rng(SEED)
    places = N_KF // LOOPS
    pts = [[S.point() for _ in range(PTS)] for _ in range(places)]
    for k in range(N_KF):
        for d in range(-6, 7):
            for p in pts[(k % places + d) % places]:
                if rng.random() < 0.75 - 0.08 * abs(d):
                    S.see(k, p, octave=int(rng.integers(0, 4)), stereo=(k % 3 == 0), depth=float(rng.uniform(0.5, 50.0)))
    mirror, mirror_ba, cull = to_device(S)
    G = covis.CovisGraph(N_KF, STRIDE)
    res = covis.update_results(covis.update_connections(G, mirror, list(range(N_KF))))
    assert (res["status"] == covis.OK).all(), np.bincount(res["status"])
    L = covis._lib()

    def events(fn, before=None):
        ts = []
        for i in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if before:
                before()
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ts.append(e0.elapsed_time(e1))
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    out = {"n_kf": N_KF, "n_pt": len(S.pt_valid), "conn_stride": STRIDE, "slots_per_kf": float(np.mean([len(s) for s in S.slots])),
           "obs_per_pt": float(np.mean([len(o) for o in S.obs])), "warmup": WARMUP, "reps": REPS}
    full = {name: t.clone() for name, t in G.t.items()}
    for n in (1, 64):
        for name, t in G.t.items():
            t.copy_(full[name])
        kfs = list(range(N_KF - n, N_KF))
        assert (covis.erase_keyframes(G, kfs).cpu().numpy() == covis.OK).all()
        torch.cuda.synchronize()
        start = {name: t.clone() for name, t in G.t.items()}
        d_kfs = torch.tensor(kfs, dtype=torch.int32, device="cuda")
        ws = torch.empty(covis.update_workspace_bytes(n, N_KF), dtype=torch.uint8, device="cuda")
        results = torch.empty((n, 32), dtype=torch.uint8, device="cuda")

        def restore():
            for name, t in G.t.items():
                t.copy_(start[name])

        def call():
            orbgpu._check(L.orbgpu_covis_update_connections_batch_device(
                n, d_kfs.data_ptr(), ctypes.byref(mirror.c), ctypes.byref(G.c), ws.data_ptr(), ws.numel(), results.data_ptr(),
                None), "update_connections")

        out[f"update_{n}"] = events(call, restore)
        r = covis.update_results(results)
        assert (r["status"] == covis.OK).all()
        if n == 1:
            out["update_1_counted"], out["update_1_ordered"] = int(r["n_counted"][0]), int(r["n_ordered"][0])
    for name, t in G.t.items():
        t.copy_(full[name])
    C = covis.Culling(G, [(N_KF - 1, 0)], STRIDE, None, "cuda")

    def call():
        orbgpu._check(L.orbgpu_covis_keyframe_culling_batch_device(
            1, C.jobs.data_ptr(), ctypes.byref(mirror.c), ctypes.byref(mirror_ba.c), ctypes.byref(cull.c), ctypes.byref(G.c),
            STRIDE, C.results.data_ptr(), C.verdicts.data_ptr(), C.culled.data_ptr(), None), "keyframe_culling")

    out["culling"] = events(call)
    r = C.host()[0]
    assert int(r["status"][0]) == covis.OK
    out["cull_list"], out["cull_culled"] = int(r["n_list"][0]), int(r["n_culled"][0])
    line = json.dumps(out)
    print(line)
    print(row(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n" + row(out) + "\n")


if __name__ == "__main__":
    main()
