"""The covisibility graph as a table in HBM (include/orbgpu_covis.h,
csrc/covis.hip), beside a ``track.MapMirror`` and a ``localba.MapMirrorBA``.

* ``CovisGraph`` -- the table: per keyframe the connected keyframes and weights
  in map order, the ordered list and the best 10.  ``upload`` fills it from host
  lists, ``download`` / ``lists`` bring it back, ``attach`` points a
  ``MapMirrorBA``'s covis_all at it, so the LBA gather reads the lists where they
  are kept.
* ``erase_keyframes`` -- the covisibility part of KeyFrame::SetBadFlag for a
  list of keyframes, asynchronous on the given stream.
* ``update_connections`` -- KeyFrame::UpdateConnections for a list of keyframes
  against a ``track.MapMirror``.
* ``keyframe_culling`` -- the judging loop of LocalMapping::KeyFrameCulling
  against the two mirrors and a ``MapMirrorCull``; ``Culling.erase`` hands its
  culled rows to the erasure on the same stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu

OK, EMPTY, CAPACITY, BAD_JOB = 0, 1, 2, 3              # ORBGPU_COVIS_*
KEPT, CULLED, TO_BE_ERASED, SKIPPED_FIRST = 0, 1, 2, 3 # ORBGPU_COVIS_CULL_*
BEST, MAX_STRIDE, TH = 10, 1024, 15                    # ORBGPU_COVIS_BEST, _MAX_STRIDE, _TH
_vp, _i = ctypes.c_void_p, ctypes.c_int
_BOUND = False


class CovisGraphStruct(ctypes.Structure):
    _fields_ = [("n_kf", _i), ("conn_stride", _i), ("n_conn", _vp), ("conn_kf", _vp), ("conn_w", _vp), ("n_ord", _vp),
                ("ord_kf", _vp), ("ord_w", _vp), ("covis10", _vp)]


class UpdateResult(ctypes.Structure):
    _fields_ = [("status", _i), ("n_counted", _i), ("n_ordered", _i), ("kf_max", _i), ("w_max", _i), ("front", _i),
                ("pad", _i * 2)]


class MapMirrorCullStruct(ctypes.Structure):
    _fields_ = [("kp_octave", _vp), ("kp_depth", _vp), ("kf_th_depth", _vp), ("kf_not_erase", _vp)]


class CullJob(ctypes.Structure):
    _fields_ = [("kf", _i), ("mono", _i)]


class CullVerdict(ctypes.Structure):
    _fields_ = [("kf", _i), ("n_mps", _i), ("n_redundant", _i), ("verdict", _i)]


class CullResult(ctypes.Structure):
    _fields_ = [("status", _i), ("n_list", _i), ("n_culled", _i), ("n_to_be_erased", _i), ("pad", _i * 4)]


UPDATE_RESULT_DTYPE = np.dtype([(name, "<i4") for name, _ in UpdateResult._fields_[:-1]] + [("pad", "<i4", (2,))])
CULL_VERDICT_DTYPE = np.dtype([(name, "<i4") for name, _ in CullVerdict._fields_])
CULL_RESULT_DTYPE = np.dtype([(name, "<i4") for name, _ in CullResult._fields_[:-1]] + [("pad", "<i4", (4,))])
assert UPDATE_RESULT_DTYPE.itemsize == ctypes.sizeof(UpdateResult) == 32 and ctypes.sizeof(CullJob) == 8
assert CULL_VERDICT_DTYPE.itemsize == ctypes.sizeof(CullVerdict) == 16
assert CULL_RESULT_DTYPE.itemsize == ctypes.sizeof(CullResult) == 32


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        import localba
        import track
        G, M = ctypes.POINTER(CovisGraphStruct), ctypes.POINTER(track.MapMirrorStruct)
        L.orbgpu_covis_erase_keyframes_batch_device.argtypes = [_i, _vp, G, _vp, _vp]
        L.orbgpu_covis_update_workspace_bytes.argtypes = [_i, _i]
        L.orbgpu_covis_update_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_covis_update_connections_batch_device.argtypes = [_i, _vp, M, G, _vp, ctypes.c_size_t, _vp, _vp]
        L.orbgpu_covis_keyframe_culling_batch_device.argtypes = [
            _i, _vp, M, ctypes.POINTER(localba.MapMirrorBAStruct), ctypes.POINTER(MapMirrorCullStruct), G, _i, _vp, _vp, _vp, _vp]
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


class MapMirrorCull:
    """What KeyFrameCulling's judge reads beside a track.MapMirror and a localba.MapMirrorBA, uploaded from numpy:
    kp_octave / kp_depth (per keyframe an (n_slots,) array, parallel to the mirror's slots), kf_th_depth and
    kf_not_erase (n_kf,).  The caller keeps it current."""

    def __init__(self, kp_octave, kp_depth, kf_th_depth, kf_not_erase, device="cuda"):
        import track
        flat = lambda rows, dt: np.concatenate([np.asarray(r, dt).reshape(-1) for r in rows] + [np.zeros(0, dt)])
        host = {"kp_octave": (flat(kp_octave, np.uint8), np.uint8), "kp_depth": (flat(kp_depth, np.float32), np.float32),
                "kf_th_depth": (kf_th_depth, np.float32), "kf_not_erase": (kf_not_erase, np.uint8)}
        self.t = {name: track._up(a, dt, device) for name, (a, dt) in host.items()}
        c = self.c = MapMirrorCullStruct()
        for name, t in self.t.items():
            setattr(c, name, track._ptr(t))


def update_workspace_bytes(n: int, n_kf: int) -> int:
    return int(_lib().orbgpu_covis_update_workspace_bytes(n, n_kf))


def _on(stream):
    import contextlib
    import torch
    return torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else contextlib.nullcontext()


def update_connections(graph, mirror, kfs, stream=None, device="cuda"):
    """orbgpu_covis_update_connections_batch_device for `kfs` in order on `graph` against the track.MapMirror
    `mirror`; returns the results, a (n, 32) uint8 tensor to view as UPDATE_RESULT_DTYPE once downloaded"""
    import torch
    n = len(kfs)
    need = update_workspace_bytes(n, graph.n_kf)
    if n > 0 and need == 0:
        raise ValueError("n * n_kf does not fit an int")
    with _on(stream):  # the list is copied and the buffers allocated on the stream the launches run on
        d_kfs = torch.from_numpy(np.asarray(list(kfs) + [0] * (n == 0), np.int32)).to(device)
        results = torch.empty((max(n, 1), ctypes.sizeof(UpdateResult)), dtype=torch.uint8, device=device)  # every one is written
        ws = torch.empty((max(need, 4),), dtype=torch.uint8, device=device)
    orbgpu._check(_lib().orbgpu_covis_update_connections_batch_device(
        n, orbgpu._ptr(d_kfs), ctypes.byref(mirror.c), ctypes.byref(graph.c), orbgpu._ptr(ws), ws.numel(), orbgpu._ptr(results),
        orbgpu._stream_ptr(stream)), "orbgpu_covis_update_connections_batch_device")
    graph._update = (d_kfs, ws, mirror)  # stay allocated while the launches are in flight on another stream
    return results[:n]


def update_results(results) -> np.ndarray:
    """the downloaded results of update_connections as a record array"""
    return results.cpu().numpy().reshape(-1).view(UPDATE_RESULT_DTYPE)


class Culling:
    """The buffers of one orbgpu_covis_keyframe_culling_batch_device call: results (n, 32) uint8, verdicts
    (n, list_stride, 4) int32 and culled (n, list_stride) int32, which erase() hands unchanged to
    orbgpu_covis_erase_keyframes_batch_device on the same stream."""

    def __init__(self, graph, jobs, list_stride, stream, device, guard=None):
        """guard: a byte to fill verdicts with before the launch, for a test of what the launch leaves alone"""
        import torch
        self.graph, self.n, self.list_stride, self.stream = graph, len(jobs), int(list_stride), stream
        n = max(self.n, 1)
        tab = np.zeros((n, 2), np.int32)
        tab[:self.n] = np.asarray([(int(kf), int(bool(mono))) for kf, mono in jobs], np.int32).reshape(-1, 2)
        with _on(stream):
            self.jobs = torch.from_numpy(tab).to(device)
            self.results = torch.empty((n, ctypes.sizeof(CullResult)), dtype=torch.uint8, device=device)
            self.verdicts = torch.empty((n, self.list_stride, 4), dtype=torch.int32, device=device)
            self.culled = torch.empty((n, self.list_stride), dtype=torch.int32, device=device)
            self.status = torch.empty((n * self.list_stride,), dtype=torch.int32, device=device)
            if guard is not None:
                self.verdicts.view(torch.uint8).fill_(guard)

    def erase(self):
        """the graph side of the culled keyframes' SetBadFlag, with no download between the two calls; returns the
        erasure's status per entry of `culled` (BAD_JOB where it holds -1)"""
        m = self.n * self.list_stride
        orbgpu._check(_lib().orbgpu_covis_erase_keyframes_batch_device(
            m, orbgpu._ptr(self.culled), ctypes.byref(self.graph.c), orbgpu._ptr(self.status), orbgpu._stream_ptr(self.stream)),
            "orbgpu_covis_erase_keyframes_batch_device")
        return self.status[:m]

    def host(self):
        """(results as a record array, verdicts as a (n, list_stride) record array, culled) downloaded"""
        r = self.results.cpu().numpy().reshape(-1).view(CULL_RESULT_DTYPE)[:self.n]
        v = self.verdicts.cpu().numpy().reshape(-1).view(CULL_VERDICT_DTYPE).reshape(-1, self.list_stride)[:self.n]
        return r, v, self.culled.cpu().numpy()[:self.n]


def keyframe_culling(graph, mirror, mirror_ba, cull_mirror, jobs, stream=None, list_stride=None, device="cuda", guard=None):
    """orbgpu_covis_keyframe_culling_batch_device for `jobs`, (kf, mono) pairs, each judged on its own; returns a
    Culling.  list_stride: the graph's conn_stride when None."""
    c = Culling(graph, jobs, graph.conn_stride if list_stride is None else list_stride, stream, device, guard)
    orbgpu._check(_lib().orbgpu_covis_keyframe_culling_batch_device(
        c.n, orbgpu._ptr(c.jobs), ctypes.byref(mirror.c), ctypes.byref(mirror_ba.c), ctypes.byref(cull_mirror.c),
        ctypes.byref(graph.c), c.list_stride, orbgpu._ptr(c.results), orbgpu._ptr(c.verdicts), orbgpu._ptr(c.culled),
        orbgpu._stream_ptr(stream)), "orbgpu_covis_keyframe_culling_batch_device")
    c.mirrors = (mirror, mirror_ba, cull_mirror)  # stay allocated while the launch is in flight
    return c
