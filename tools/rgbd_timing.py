"""RGB-D input kernels on one MI355X (csrc/rgbd.hip), beside a same-run copy.

gray_from_color_batch at B frames of W x H, for RGB (pitch 3*W) and RGBA, on
the 16-byte path and on the general path (the same frames from a source base
pointer one byte off 16-byte alignment): median of event-timed launches, the
bytes the conversion has to move (source pixels read + grey bytes written)
over that time, the same for a plain device-to-device torch copy that moves
the same total (it copies half of it: every copied byte is read and written),
the kernel-to-copy ratio, and the fraction of the 8 TB/s HBM peak the
project's roofline uses.  stereo_from_rgbd_batch at --keypoints per frame is
reported the same way.  The 16-byte and general outputs are compared with each
other and, for one frame, with the formula evaluated in numpy.

Prints one JSON document and writes it to --out.

usage: python tools/rgbd_timing.py [--batch 512] [--width 640] [--height 480] [--launches 60] [--warmup 10]
                                   [--out profiles/rgbd_timing.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "orb-slam2-annotation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbgpu  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, the roofline of DESIGN.md §4


def timed(fn, launches, warmup):
    """median / min / max milliseconds of `launches` event-timed calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return statistics.median(ms), min(ms), max(ms)


def report(name, nbytes, ms, copy_ms):
    med, lo, hi = ms
    cmed = copy_ms[0]
    return {"case": name, "bytes_moved": nbytes, "ms_median": round(med, 4), "ms_min": round(lo, 4),
            "ms_max": round(hi, 4), "bytes_per_s": round(nbytes / (med * 1e-3), 0),
            "copy_ms_median": round(cmed, 4), "copy_bytes_per_s": round(nbytes / (cmed * 1e-3), 0),
            "kernel_to_copy_time_ratio": round(med / cmed, 3),
            "fraction_of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}


def copy_yardstick(total_bytes, launches, warmup):
    """a torch copy that reads total/2 and writes total/2 bytes"""
    n = total_bytes // 2
    a = torch.empty(n, dtype=torch.uint8, device="cuda").random_(0, 256)
    b = torch.empty_like(a)
    return timed(lambda: b.copy_(a), launches, warmup)


def numpy_gray(px, r_pos, b_pos):
    p = px.astype(np.uint32)
    return ((p[..., r_pos] * 4899 + p[..., 1] * 9617 + p[..., b_pos] * 1868 + 8192) >> 14).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rgbd_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rgbd_timing needs a GPU"
    assert a.launches >= 50, "the median is taken over at least 50 launches"
    B, W, H = a.batch, a.width, a.height
    assert W % 16 == 0, "the timed shapes keep the 16-byte path's alignment"
    results = []
    for code, name, ch in ((orbgpu.COLOR_RGB, "rgb", 3), (orbgpu.COLOR_RGBA, "rgba", 4)):
        n_src = B * H * W * ch
        raw = torch.empty(n_src, dtype=torch.uint8, device="cuda").random_(0, 256)
        off1 = torch.empty(n_src + 16, dtype=torch.uint8, device="cuda")
        off1[1:n_src + 1] = raw  # the same frames one byte off alignment
        views = {"fast": torch.as_strided(raw, (B, H, W * ch), (H * W * ch, W * ch, 1), 0),
                 "general": torch.as_strided(off1, (B, H, W * ch), (H * W * ch, W * ch, 1), 1)}
        assert views["fast"].data_ptr() % 16 == 0 and views["general"].data_ptr() % 16 == 1
        gray = {k: torch.zeros((B, H, W), dtype=torch.uint8, device="cuda") for k in views}
        total = n_src + B * H * W
        copy_ms = copy_yardstick(total, a.launches, a.warmup)
        for path in ("fast", "general"):
            ms = timed(lambda: orbgpu.gray_from_color_batch(views[path], code, gray[path], width=W),
                       a.launches, a.warmup)
            results.append(report(f"gray_{name}_{path}", total, ms, copy_ms))
        assert torch.equal(gray["fast"], gray["general"]), "16-byte and general path differ"
        f = B - 1
        want = numpy_gray(views["fast"][f].cpu().numpy().reshape(H, W, ch), 0, 2)
        assert np.array_equal(gray["fast"][f].cpu().numpy(), want), "grey differs from the formula"
        del raw, off1, views, gray
        torch.cuda.empty_cache()

    # stereo_from_rgbd_batch: uint16 maps, TUM factor, `keypoints` per frame
    N = a.keypoints
    rng = np.random.default_rng(1)
    k = np.zeros((B, N), orbgpu.KP_DTYPE)
    k["x"], k["y"] = rng.uniform(0, W - 1, (B, N)), rng.uniform(0, H - 1, (B, N))
    kps = torch.from_numpy(k.view(np.float32).reshape(B, N, 7).copy()).cuda()
    kps_un = kps.clone()
    counts = torch.full((B,), N, dtype=torch.int32, device="cuda")
    maps = torch.randint(0, 30000, (B, H, W), dtype=torch.int32, device="cuda").to(torch.int16)
    cam = orbgpu.Camera.make(517.306408, 516.469215, 318.643040, 255.313989, [0.0, 0.0, 0.0, 0.0])
    uright, depth = (torch.zeros((B, N), dtype=torch.float32, device="cuda") for _ in range(2))
    x3dc = torch.zeros((B, N, 3), dtype=torch.float32, device="cuda")
    total = B * N * (2 * 28 + 2 + 8 + 12)  # two keypoints and a sample read, five floats written
    copy_ms = copy_yardstick(total, a.launches, a.warmup)
    ms = timed(lambda: orbgpu.stereo_from_rgbd_batch(maps, 1.0 / 5000.0, kps, kps_un, counts, cam, 40.0, uright,
                                                     depth, x3dc), a.launches, a.warmup)
    results.append(report("stereo_from_rgbd_u16_x3dc", total, ms, copy_ms))
    assert 0.5 < (depth > 0).float().mean().item() <= 1.0

    doc = {"tool": "tools/rgbd_timing.py", "device": orbgpu.device_arch(),
           "shape": {"batch": B, "width": W, "height": H, "keypoints_per_frame": N},
           "timing": f"median of {a.launches} event-timed launches after {a.warmup} warm-up launches; "
                     "copy = torch Tensor.copy_ device to device moving the same total bytes, same process",
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text + "\n")


if __name__ == "__main__":
    main()
