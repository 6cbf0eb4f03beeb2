#!/usr/bin/env python3
"""Where fast_cells_kernel's per-cell work goes, counted on the CPU.

Restates in numpy what csrc/fast.hip computes per cell -- the cell grid of
csrc/geometry.cpp, the compass pre-test, the arc strength (cornerScore + 1),
the 3x3 NMS that decides the minThFAST retry, and the row bands of the
survivor list -- and counts survivors, corners and arc-pass chunks per cell on
the bench stream (levels from the oracle extractor).  Prints the table of
DESIGN section 10's arc-chunk row and the predicted arc-pass VALU per cell
with and without the 64-entry tail chunk, under the two chunk costs read from
the gfx950 disassembly.  Needs the oracle library (oracle/liborbref.so) and
numpy; no GPU.

    python3 tools/fast_cell_stats.py [--frames 3] [--t0 37] [--full-cost 125] [--half-cost 65]

tests/test_fast_tail_chunks.py uses level_cells / compass_strength /
list_len to check that its frames reach every chunk-boundary case.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT / "orb-slam2-annotation_amd", ROOT / "oracle"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

K_EDGE = 19          # EDGE_THRESHOLD
K_BORDER = K_EDGE - 3  # minBorderX / minBorderY
# 64 / ng of fast.hip's dword compass (c_ng_rpi)
NG_RPI = [0, 64, 32, 21, 16, 12, 10, 9, 8, 7, 6, 5, 5, 4, 4, 4, 4, 3]


def level_cells(w: int, h: int):
    """The FAST cells of a w x h level (geometry.cpp, fast.hip): a list of
    dicts with the detection region [x0, x1) x [y0, y1) in level pixels, the
    cell size (wcell, hcell) and iniX (the window's first column)."""
    max_bx, max_by = w - K_EDGE + 3, h - K_EDGE + 3
    width, height = np.float32(max_bx - K_BORDER), np.float32(max_by - K_BORDER)
    ncols, nrows = int(width / np.float32(30)), int(height / np.float32(30))
    wcell, hcell = int(np.ceil(width / np.float32(ncols))), int(np.ceil(height / np.float32(nrows)))
    cells = []
    for ci in range(nrows):
        for cj in range(ncols):
            ini_y, ini_x = K_BORDER + ci * hcell, K_BORDER + cj * wcell
            if ini_y >= max_by - 3 or ini_x >= max_bx - 6:
                continue
            max_y, max_x = min(ini_y + hcell + 6, max_by), min(ini_x + wcell + 6, max_bx)
            if max_x - ini_x - 6 <= 0 or max_y - ini_y - 6 <= 0:
                continue
            cells.append(dict(x0=ini_x + 3, x1=max_x - 3, y0=ini_y + 3, y1=max_y - 3, ini_x=ini_x,
                              wcell=wcell, hcell=hcell))
    return cells


def list_len(level_sizes) -> int:
    """Entries of a cell wave's survivor list for an extractor whose levels
    have the given (w, h) sizes: geometry.cpp's window pitch / rows /
    det_max and fast.hip's fast_list_len (ORBGPU_FAST_BANDS)."""
    pitch = rows = det_max = 0
    for w, h in level_sizes:
        c = level_cells(w, h)[0]
        pitch = max(pitch, (c["wcell"] + 11 + 3) // 4 * 4)
        rows = max(rows, c["hcell"] + 6)
        det_max = max(det_max, (c["wcell"] * c["hcell"] + 7) // 8 * 8)
    pitch = 40 if pitch <= 40 else (pitch + 7) // 8 * 8
    c = ((4864 - 2 * pitch * rows - 16) // 2 - 1) & ~7
    return det_max if c >= det_max else (c if c >= 256 else det_max)


def _shift(img: np.ndarray, dx: int, dy: int) -> np.ndarray:
    """img[y + dy, x + dx] for the interior pixels (3-px margin)"""
    h, w = img.shape
    return img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]


def compass_strength(img: np.ndarray) -> np.ndarray:
    """fast.hip's compass pre-test value per pixel (a pixel survives at
    threshold t iff it exceeds t): with the compass points c0 / c8 (3 below /
    above) and c4 / c12 (3 right / left), the smallest pairwise max of adjacent
    points is max(min(c0, c8), min(c4, c12)), the largest pairwise min is
    min(max(c0, c8), max(c4, c12)).  Full-size array, 0 in the 3-px margin."""
    i = img.astype(np.int16)
    v, c0, c8, c4, c12 = _shift(i, 0, 0), _shift(i, 0, 3), _shift(i, 0, -3), _shift(i, 3, 0), _shift(i, -3, 0)
    dark = np.maximum(np.minimum(c0, c8), np.minimum(c4, c12))
    bright = np.minimum(np.maximum(c0, c8), np.maximum(c4, c12))
    out = np.zeros(img.shape, np.int16)
    out[3:-3, 3:-3] = np.maximum(np.maximum(v - dark, 0), np.maximum(bright - v, 0))
    return out


RING_DX = [0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1]
RING_DY = [3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3]


def arc_strength(img: np.ndarray) -> np.ndarray:
    """cornerScore + 1 per pixel: max(v - min_k max9_k, max_k min9_k - v) over
    the 16 9-arcs of the ring (a corner at t iff >= t + 1).  Full-size int16
    array, 0 in the 3-px margin."""
    i = img.astype(np.int16)
    ring = [_shift(i, dx, dy) for dx, dy in zip(RING_DX, RING_DY)]
    hi3 = [np.maximum(np.maximum(ring[k], ring[(k + 1) % 16]), ring[(k + 2) % 16]) for k in range(16)]
    lo3 = [np.minimum(np.minimum(ring[k], ring[(k + 1) % 16]), ring[(k + 2) % 16]) for k in range(16)]
    a = b = None
    for k in range(16):
        hi9 = np.maximum(np.maximum(hi3[k], hi3[(k + 3) % 16]), hi3[(k + 6) % 16])
        lo9 = np.minimum(np.minimum(lo3[k], lo3[(k + 3) % 16]), lo3[(k + 6) % 16])
        a = hi9 if a is None else np.minimum(a, hi9)
        b = lo9 if b is None else np.maximum(b, lo9)
    v = _shift(i, 0, 0)
    out = np.zeros(img.shape, np.int16)
    out[3:-3, 3:-3] = np.maximum(v - a, b - v)
    return out


def survivors_with_ring8(img: np.ndarray, t: int) -> np.ndarray:
    """compass survivors that also pass the strongest 8-point test: 4
    consecutive even ring positions all brighter than v + t or all darker
    than v - t (a 9-arc contains 4 such positions)."""
    i = img.astype(np.int16)
    v = _shift(i, 0, 0)
    ev = [_shift(i, RING_DX[k], RING_DY[k]) for k in range(0, 16, 2)]
    ok = np.zeros(v.shape, bool)
    for k in range(8):
        q = [ev[(k + j) % 8] for j in range(4)]
        ok |= (np.minimum(np.minimum(q[0], q[1]), np.minimum(q[2], q[3])) > v + t)
        ok |= (np.maximum(np.maximum(q[0], q[1]), np.maximum(q[2], q[3])) < v - t)
    out = np.zeros(img.shape, bool)
    out[3:-3, 3:-3] = ok
    return out & (compass_strength(img) > t)


def cell_survivors(img: np.ndarray, t: int, cells=None) -> np.ndarray:
    """compass survivors at threshold t per cell of the level image"""
    cells = level_cells(img.shape[1], img.shape[0]) if cells is None else cells
    m = compass_strength(img) > t
    return np.array([int(m[c["y0"]:c["y1"], c["x0"]:c["x1"]].sum()) for c in cells], np.int64)


def _nms_count(score: np.ndarray, t: int) -> int:
    """keypoints cv::FAST(nonmax) keeps in a cell: corners (score > t) strictly
    above their 8 neighbours, non-corners and pixels outside the region 0"""
    s = np.where(score > t, score, 0)
    p = np.pad(s, 1)
    h, w = s.shape
    nb = np.max([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], axis=0)
    return int(((s > 0) & (s > nb)).sum())


def band_chunks(surv_rows, corner_rows, dw: int, ini_x: int, dump: int):
    """Arc-pass chunk sizes of one threshold pass of a cell as
    fast_cell_banded runs it: the compass fills the list in row bands (rpi rows
    per iteration, a band ends when an iteration might not fit), each band's
    survivors go through the arc pass, and corners whose neighbourhood is not
    complete yet stay pending at the front of the list.  Returns the list of
    the bands' survivor counts."""
    xa = ini_x & ~3
    ox = ini_x - xa + ((1 - (ini_x - xa)) & 3)
    c_lo = 3 + ox
    ng = ((c_lo + dw - 1) >> 2) - (c_lo >> 2) + 1
    rpi = NG_RPI[ng]
    dh = len(surv_rows)
    out, nb, row = [], 0, 0
    while True:
        na, rr = nb, row
        while rr < dh and na + dw * rpi <= dump:
            na += int(surv_rows[rr:rr + rpi].sum())
            rr += rpi
        assert rr > row, "a band made no progress"
        out.append(na - nb)
        row = rr
        if row >= dh:
            return out
        nb = int(corner_rows[row - 1])  # the corners of region rows >= row - 1 stay pending


def chunk_split(n: int):
    """(full, half) chunks of an arc pass over n entries with the 64-entry
    tail chunk: full chunks while 65 or more remain, then one half chunk"""
    full = 0
    while n > 64:
        full += 1
        n -= 128
    return full, 1 if n > 0 else 0


def frame_stats(levels, ini_th: int = 20, min_th: int = 7):
    """per-cell records of one frame's levels"""
    dump = list_len([(im.shape[1], im.shape[0]) for im in levels])
    recs = []
    for l, img in enumerate(levels):
        comp, arc = compass_strength(img), arc_strength(img)
        s8 = survivors_with_ring8(img, ini_th)
        for c in level_cells(img.shape[1], img.shape[0]):
            sl = (slice(c["y0"], c["y1"]), slice(c["x0"], c["x1"]))
            cm, sc = comp[sl], arc[sl]
            surv = cm > ini_th
            corner = surv & (sc > ini_th)
            rec = dict(level=l, pixels=cm.size, s4=int(surv.sum()), s8=int(s8[sl].sum()), corners=int(corner.sum()),
                       bands=band_chunks(surv.sum(axis=1), corner.sum(axis=1), cm.shape[1], c["ini_x"], dump),
                       retry=_nms_count(np.where(surv, sc, 0), ini_th) == 0)
            if rec["retry"]:
                surv7 = cm > min_th
                corner7 = surv7 & (sc > min_th)
                rec.update(s4_retry=int(surv7.sum()), corners_retry=int(corner7.sum()),
                           bands_retry=band_chunks(surv7.sum(axis=1), corner7.sum(axis=1), cm.shape[1], c["ini_x"], dump))
            recs.append(rec)
    return recs, dump


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--t0", type=int, default=37)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--full-cost", type=float, default=125.0, help="VALU of one 128-entry chunk (disassembly)")
    ap.add_argument("--half-cost", type=float, default=65.0, help="VALU of one 64-entry tail chunk (disassembly)")
    a = ap.parse_args()
    import orbref
    import synth

    frames = synth.torch_stream(a.frames, a.width, a.height, device="cpu", bounded=True, t0=a.t0).numpy()
    ref = orbref.Extractor(nfeatures=a.nfeatures)
    recs = []
    for img in frames:
        ref.extract(np.ascontiguousarray(img[:, :a.width]))
        r, dump = frame_stats([ref.level(l) for l in range(8)])
        recs += r
    n = len(recs)
    s4 = np.array([r["s4"] for r in recs])
    naive = -(-s4 // 128)
    naive8 = -(-np.array([r["s8"] for r in recs]) // 128)
    retry = [r for r in recs if r["retry"]]
    print(f"{n} cells ({n / a.frames:.0f} per frame), survivor list {dump} entries")
    print(f"detection pixels per cell            {np.mean([r['pixels'] for r in recs]):.0f}")
    print(f"compass survivors at t = 20 (s4)     {s4.mean():.1f} per cell "
          f"({100 * s4.sum() / sum(r['pixels'] for r in recs):.0f} % of pixels)")
    print(f"corners before NMS at t = 20         {np.mean([r['corners'] for r in recs]):.1f} per cell "
          f"({100 * sum(r['corners'] for r in recs) / max(s4.sum(), 1):.0f} % of survivors)")
    print(f"arc chunks per cell, ceil(s4 / 128)  {naive.mean():.2f}")
    print("cells by chunk count 0..6+           " + " / ".join(str(int((naive == k).sum())) for k in range(6))
          + f" / {int((naive >= 6).sum())}")
    tail = s4 % 128
    print(f"cells with s4 % 128 in (0, 64]       {100 * ((tail > 0) & (tail <= 64)).mean():.1f} %")
    print(f"cells that retry at minThFAST        {100 * len(retry) / n:.1f} %")
    if retry:
        print(f"  survivors per retrying cell, t = 20  {np.mean([r['s4'] for r in retry]):.0f}")
        print(f"  survivors per retrying cell, t = 7   {np.mean([r['s4_retry'] for r in retry]):.0f} "
              f"({np.mean([r['corners_retry'] for r in retry]):.1f} corners)")
    print(f"survivors with an 8-point ring test  {np.mean([r['s8'] for r in recs]):.0f} per cell, "
          f"{naive8.mean():.2f} chunks per cell")
    # arc-pass VALU per cell, bands and retry passes included
    passes = [b for r in recs for b in r["bands"] + r.get("bands_retry", [])]
    old_chunks = sum(-(-b // 128) for b in passes)
    full = sum(chunk_split(b)[0] for b in passes)
    half = sum(chunk_split(b)[1] for b in passes)
    old = old_chunks * a.full_cost / n
    new = (full * a.full_cost + half * a.half_cost) / n
    multi = sum(len(r["bands"]) > 1 for r in recs)
    print(f"cells whose first pass needs more than one band: {multi} ({100 * multi / n:.1f} %)")
    print(f"arc passes as the kernel runs them (bands, retries): {old_chunks / n:.2f} chunks per cell; "
          f"with the tail chunk {full / n:.2f} full + {half / n:.2f} half")
    print(f"arc-pass VALU per cell at {a.full_cost:g} / {a.half_cost:g} per chunk: {old:.1f} -> {new:.1f} "
          f"({new - old:+.1f})")
    print(f"per 512-frame launch ({n / a.frames:.0f} cells per frame): {(new - old) * n / a.frames * 512 / 1e6:+.1f} M VALU")


if __name__ == "__main__":
    main()
