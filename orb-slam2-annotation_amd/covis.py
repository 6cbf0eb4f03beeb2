"""The covisibility graph as a table in HBM (include/orbgpu_covis.h,
csrc/covis.hip), beside a ``track.MapMirror`` and a ``localba.MapMirrorBA``.

* ``CovisGraph`` -- the table: per keyframe the connected keyframes and weights
  in map order, the ordered list and the best 10.  ``upload`` fills it from host
  lists, ``download`` / ``lists`` bring it back, ``attach`` points a
  ``MapMirrorBA``'s covis_all at it, so the LBA gather reads the lists where they
  are kept.
* ``erase_keyframes`` -- the covisibility part of KeyFrame::SetBadFlag for a
  list of keyframes, asynchronous on the given stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu

OK, BAD_JOB = 0, 3                                     # ORBGPU_COVIS_*
BEST, MAX_STRIDE = 10, 1024                            # ORBGPU_COVIS_BEST, _MAX_STRIDE
_vp, _i = ctypes.c_void_p, ctypes.c_int
_BOUND = False


class CovisGraphStruct(ctypes.Structure):
    _fields_ = [("n_kf", _i), ("conn_stride", _i), ("n_conn", _vp), ("conn_kf", _vp), ("conn_w", _vp), ("n_ord", _vp),
                ("ord_kf", _vp), ("ord_w", _vp), ("covis10", _vp)]


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        L.orbgpu_covis_erase_keyframes_batch_device.argtypes = [_i, _vp, ctypes.POINTER(CovisGraphStruct), _vp, _vp]
        _BOUND = True
    return L


def ordered(conn):
    """UpdateBestCovisibles: a row of (keyframe, weight) pairs in map order, sorted as std::sort on (weight,
    KeyFrame*) and reversed -- the position in the row stands for the pointer"""
    return [conn[i] for _, i in sorted(((w, i) for i, (_, w) in enumerate(conn)), reverse=True)]


class CovisGraph:
    """The table of n_kf rows of conn_stride entries.  covis10: a tensor to use for the best 10 in place of one
    of its own, such as a track.MapMirror's t["covis"]."""

    ROWS = ("conn_kf", "conn_w", "ord_kf", "ord_w")

    def __init__(self, n_kf, conn_stride, device="cuda", covis10=None):
        import torch
        self.n_kf, self.conn_stride = int(n_kf), int(conn_stride)
        n, S = max(self.n_kf, 1), max(self.conn_stride, 1)
        z = lambda shape: torch.zeros(shape, dtype=torch.int32, device=device)
        t = self.t = {"n_conn": z((n,)), "n_ord": z((n,))}
        for name in self.ROWS:
            t[name] = z((n, S))
        if covis10 is None:
            covis10 = torch.full((n, BEST), -1, dtype=torch.int32, device=device)
        assert covis10.numel() * covis10.element_size() >= 4 * BEST * self.n_kf
        t["covis10"] = covis10
        c = self.c = CovisGraphStruct()
        c.n_kf, c.conn_stride = self.n_kf, self.conn_stride
        for name, x in t.items():
            setattr(c, name, x.data_ptr())

    def download(self) -> dict:
        """every array as numpy, rows as (n_kf, conn_stride), covis10 as (n_kf, 10)"""
        out = {name: x.cpu().numpy() for name, x in self.t.items()}
        out["covis10"] = out["covis10"].reshape(-1).view(np.uint8)[:4 * BEST * max(self.n_kf, 1)].view(np.int32).reshape(-1, BEST)
        return out

    def lists(self):
        """(conn, ord): per keyframe the (keyframe, weight) pairs of both rows"""
        h = self.download()
        pairs = lambda kf, w, n: [[(int(kf[k, i]), int(w[k, i])) for i in range(int(n[k]))] for k in range(self.n_kf)]
        return pairs(h["conn_kf"], h["conn_w"], h["n_conn"]), pairs(h["ord_kf"], h["ord_w"], h["n_ord"])

    def upload(self, conn, ord=None) -> None:
        """conn: per keyframe its (keyframe, weight) pairs in map order; ord: the ordered pairs, computed from
        conn when None.  Only the counts, the entries below them and the best 10 are written."""
        import torch
        h = self.download()
        for k in range(self.n_kf):
            o = ordered(conn[k]) if ord is None else ord[k]
            for rows, cnt, a, b in ((conn[k], "n_conn", "conn_kf", "conn_w"), (o, "n_ord", "ord_kf", "ord_w")):
                assert len(rows) <= self.conn_stride
                h[cnt][k] = len(rows)
                for i, (kf, w) in enumerate(rows):
                    h[a][k, i], h[b][k, i] = kf, w
            best = [kf for kf, _ in o[:BEST]]
            h["covis10"][k] = best + [-1] * (BEST - len(best))
        for name, x in self.t.items():
            src = torch.from_numpy(np.ascontiguousarray(h[name]).reshape(-1).view(np.uint8).copy())
            x.view(-1).view(torch.uint8)[:src.numel()].copy_(src.to(x.device))

    def attach(self, mirror_ba) -> None:
        """point a localba.MapMirrorBA's covis_all at the ordered rows: the lists are read where they are kept"""
        import torch
        self._offsets = torch.arange(max(self.n_kf, 1), dtype=torch.int32, device=self.t["n_ord"].device) * self.conn_stride
        b = mirror_ba.c
        b.n_covis_all_total = self.n_kf * self.conn_stride
        b.covis_all_offset = self._offsets.data_ptr()
        b.n_covis_all = self.t["n_ord"].data_ptr()
        b.covis_all = self.t["ord_kf"].data_ptr()
        mirror_ba.graph = self  # keeps the table alive with the mirror


def erase_keyframes(graph, kfs, stream=None, device="cuda"):
    """orbgpu_covis_erase_keyframes_batch_device for `kfs` in order; returns the status per keyframe, a tensor"""
    import contextlib
    import torch
    n = len(kfs)
    # the list is copied and the status allocated on the stream the launch runs on
    with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else contextlib.nullcontext():
        d_kfs = torch.from_numpy(np.asarray(list(kfs) + [0] * (n == 0), np.int32)).to(device)
        status = torch.empty((max(n, 1),), dtype=torch.int32, device=device)  # every entry is written
    orbgpu._check(_lib().orbgpu_covis_erase_keyframes_batch_device(
        n, orbgpu._ptr(d_kfs), ctypes.byref(graph.c), orbgpu._ptr(status), orbgpu._stream_ptr(stream)),
        "orbgpu_covis_erase_keyframes_batch_device")
    graph._erased = d_kfs  # the list stays allocated while the launch is in flight on another stream
    return status[:n]
