"""Host-side mirror of the local bundle adjustment over the C ABI in
include/orbgpu_localba.h (Optimizer::LocalBundleAdjustment, src/Optimizer.cpp:
536-885; the kernel is csrc/localba.hip).

* ``local_ba_batch`` -- the host form on numpy arrays: many keyframe
  neighbourhoods in one launch.
* ``local_ba_batch_device`` -- the device form on torch tensors, asynchronous
  on a stream, with a caller-provided workspace.
* ``local_bundle_adjustment`` -- one neighbourhood: (Tcw of the local poses,
  Xw, erase, result).
* ``local_ba_chip`` / ``local_ba_chip_device`` / ``chip_workspace_bytes`` -- one
  neighbourhood spread over the whole chip (include/orbgpu_localba_chip.h,
  csrc/localba_chip.hip), synchronous, with the stop flag polled as g2o polls
  it; ``MapLocalBA.solve(chip=True)`` is the same between gather and collect.
* ``make_jobs`` / ``make_batch`` -- job records, and the concatenated arrays of
  a list of problems.
* ``MapMirrorBA`` / ``MapLocalBA`` -- against a ``track.MapMirror``
  (include/orbgpu_localba_map.h, csrc/localba_map.hip): the gather of the
  arrays from the map, the solve above and the collection of vToErase with the
  write-back into the mirror, three calls on one stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu


class LocalBAJob(ctypes.Structure):
    _fields_ = [("n_poses", ctypes.c_int), ("n_local", ctypes.c_int), ("n_points", ctypes.c_int),
                ("n_edges", ctypes.c_int), ("pose_offset", ctypes.c_int), ("point_offset", ctypes.c_int),
                ("edge_offset", ctypes.c_int), ("out_pose_offset", ctypes.c_int)]


class LocalBAResult(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_int), ("n_bad_first", ctypes.c_int), ("n_erase", ctypes.c_int),
                ("pad", ctypes.c_int), ("lm_iterations", ctypes.c_int * 2), ("lm_rejected", ctypes.c_int * 2)]


JOB_DTYPE = np.dtype([("n_poses", "<i4"), ("n_local", "<i4"), ("n_points", "<i4"), ("n_edges", "<i4"),
                      ("pose_offset", "<i4"), ("point_offset", "<i4"), ("edge_offset", "<i4"),
                      ("out_pose_offset", "<i4")])
RESULT_DTYPE = np.dtype([("rounds", "<i4"), ("n_bad_first", "<i4"), ("n_erase", "<i4"), ("pad", "<i4"),
                         ("lm_iterations", "<i4", (2,)), ("lm_rejected", "<i4", (2,))])
assert JOB_DTYPE.itemsize == ctypes.sizeof(LocalBAJob) == 32
assert RESULT_DTYPE.itemsize == ctypes.sizeof(LocalBAResult) == 32

# the batch arrays in the order of the C ABI: (name, dtype, columns, which total counts its rows)
INPUTS = (("Tcw", np.float32, 12, "poses"), ("fixed", np.uint8, 0, "poses"), ("cam", np.float32, 5, "poses"),
          ("Xw", np.float32, 3, "points"), ("edge_pose", np.int32, 0, "edges"), ("edge_point", np.int32, 0, "edges"),
          ("obs", np.float32, 3, "edges"), ("inv_sigma2", np.float32, 0, "edges"))
OUTPUTS = (("Tcw_out", np.float32, 16, "local"), ("Xw_out", np.float32, 3, "points"), ("erase", np.uint8, 0, "edges"))


def make_jobs(rows) -> np.ndarray:
    """JOB_DTYPE array of `rows`: an iterable of (n_poses, n_local, n_points,
    n_edges, pose_offset, point_offset, edge_offset, out_pose_offset)."""
    rows = [tuple(int(v) for v in r) for r in rows]
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        for name, v in zip(JOB_DTYPE.names, r):
            j[name] = v
    return jobs


def make_batch(problems):
    """(jobs, arrays) of a list of problems laid out back to back.  A problem is
    a mapping with Tcw (P, 3x4 or 4x4; the n_local local poses first), fixed
    (P), cam (P, 5) = fx, fy, cx, cy, bf, Xw (M, 3), pose_idx, point_idx (E;
    grouped by point), obs (E, 3), inv_sigma2 (E) and n_local.  `arrays` maps
    the names of INPUTS to the concatenated arrays."""
    rows, parts = [], {name: [] for name, *_ in INPUTS}
    po = lo = eo = oo = 0
    for s in problems:
        T = np.asarray(s["Tcw"], np.float32)
        T = T.reshape(len(T), -1, 4)[:, :3].reshape(len(T), 12)
        P, M, E, NL = len(T), len(np.asarray(s["Xw"]).reshape(-1, 3)), len(np.asarray(s["obs"]).reshape(-1, 3)), int(s["n_local"])
        rows.append((P, NL, M, E, po, lo, eo, oo))
        for name, val in (("Tcw", T), ("fixed", s["fixed"]), ("cam", s["cam"]), ("Xw", s["Xw"]),
                          ("edge_pose", s["pose_idx"]), ("edge_point", s["point_idx"]), ("obs", s["obs"]),
                          ("inv_sigma2", s["inv_sigma2"])):
            parts[name].append(val)
        po, lo, eo, oo = po + P, lo + M, eo + E, oo + NL
    arrays = {}
    for name, dtype, cols, _ in INPUTS:
        shape = (-1, cols) if cols else (-1,)
        rows_ = [np.asarray(v, dtype).reshape(shape) for v in parts[name]]
        arrays[name] = np.concatenate(rows_) if rows_ else np.zeros((0, cols) if cols else (0,), dtype)
    return make_jobs(rows), arrays


def workspace_bytes(batch: int, total_poses: int, total_points: int, total_edges: int, max_local: int) -> int:
    return int(orbgpu.lib().orbgpu_local_ba_workspace_bytes(batch, total_poses, total_points, total_edges, max_local))


def _max_local(jobs) -> int:
    return int(jobs["n_local"].max()) if len(jobs) else 0


def local_ba_batch(jobs, Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2, Tcw_out=None, Xw_out=None,
                   erase=None, total_local=None, max_local=None):
    """Host form of orbgpu_local_ba_batch.  jobs: JOB_DTYPE array; the arrays as
    make_batch returns them.  Returns (results as a RESULT_DTYPE array, Tcw_out
    (total_local, 16), Xw_out (total_points, 3), erase uint8 (total_edges));
    the outputs, when given, are updated in place (elements outside every job's
    ranges keep their values).  total_local defaults to the end of the last
    job's output range, max_local to the largest n_local."""
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    a = {}
    for (name, dtype, cols, _), val in zip(INPUTS, (Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2)):
        a[name] = np.ascontiguousarray(val, dtype).reshape((-1, cols) if cols else (-1,))
    tp, tm, te = len(a["Tcw"]), len(a["Xw"]), len(a["obs"])
    if not (len(a["fixed"]) == len(a["cam"]) == tp and len(a["edge_pose"]) == len(a["edge_point"]) == te
            and len(a["inv_sigma2"]) == te):
        raise ValueError("pose arrays need one row per pose, edge arrays one row per edge")
    if total_local is None:
        total_local = int((jobs["out_pose_offset"] + jobs["n_local"]).max()) if len(jobs) else 0
    if max_local is None:
        max_local = _max_local(jobs)
    outs = {}
    for (name, dtype, cols, _), val, rows in zip(OUTPUTS, (Tcw_out, Xw_out, erase), (total_local, tm, te)):
        shape = (rows, cols) if cols else (rows,)
        if val is None:
            val = np.zeros(shape, dtype)
        if val.dtype != dtype or val.shape != shape or not val.flags.c_contiguous:
            raise ValueError(f"{name} must be a contiguous {np.dtype(dtype).name} array of shape {shape}")
        outs[name] = val
    res = np.zeros(len(jobs), RESULT_DTYPE)
    orbgpu._check(orbgpu.lib().orbgpu_local_ba_batch(
        len(jobs), jobs.ctypes.data, tp, total_local, tm, te, max_local, *(a[n].ctypes.data for n, *_ in INPUTS),
        *(outs[n].ctypes.data for n, *_ in OUTPUTS), res.ctypes.data, None, 0), "orbgpu_local_ba_batch")
    return res, outs["Tcw_out"], outs["Xw_out"], outs["erase"]


def local_ba_batch_device(jobs, Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2, Tcw_out, Xw_out, erase,
                          results, workspace, max_local, stream=None) -> None:
    """Device form on torch tensors of one GPU: jobs uint8 (B, 32) (JOB_DTYPE
    bytes); Tcw float32 (TP, 12), fixed uint8 (TP), cam float32 (TP, 5), Xw
    float32 (TM, 3), edge_pose / edge_point int32 (TE), obs float32 (TE, 3),
    inv_sigma2 float32 (TE); Tcw_out float32 (TL, 16), Xw_out float32 (TM, 3),
    erase uint8 (TE), results uint8 (B, 32) (RESULT_DTYPE bytes); workspace: a
    contiguous uint8 tensor of at least workspace_bytes(B, TP, TM, TE,
    max_local) bytes.  Asynchronous on `stream` (default: the null stream)."""
    B, tp, tm, te, tl = jobs.shape[0], Tcw.shape[0], Xw.shape[0], obs.shape[0], Tcw_out.shape[0]
    for t, shape, name in ((jobs, (B, 32), "jobs"), (Tcw, (tp, 12), "Tcw"), (fixed, (tp,), "fixed"),
                           (cam, (tp, 5), "cam"), (Xw, (tm, 3), "Xw"), (edge_pose, (te,), "edge_pose"),
                           (edge_point, (te,), "edge_point"), (obs, (te, 3), "obs"), (inv_sigma2, (te,), "inv_sigma2"),
                           (Tcw_out, (tl, 16), "Tcw_out"), (Xw_out, (tm, 3), "Xw_out"), (erase, (te,), "erase"),
                           (results, (B, 32), "results")):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor of shape {shape}")
    if workspace.dim() != 1 or not workspace.is_contiguous() or workspace.element_size() != 1:
        raise ValueError("workspace: expected a contiguous one-dimensional uint8 tensor")
    orbgpu._check(orbgpu.lib().orbgpu_local_ba_batch_device(
        B, orbgpu._ptr(jobs), tp, tl, tm, te, int(max_local), orbgpu._ptr(Tcw), orbgpu._ptr(fixed), orbgpu._ptr(cam),
        orbgpu._ptr(Xw), orbgpu._ptr(edge_pose), orbgpu._ptr(edge_point), orbgpu._ptr(obs), orbgpu._ptr(inv_sigma2),
        orbgpu._ptr(Tcw_out), orbgpu._ptr(Xw_out), orbgpu._ptr(erase), orbgpu._ptr(results), orbgpu._ptr(workspace),
        workspace.numel(), orbgpu._stream_ptr(stream)), "orbgpu_local_ba_batch_device")


def local_bundle_adjustment(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local):
    """Optimizer::LocalBundleAdjustment of one neighbourhood.  Returns (Tcw
    (n_local, 4, 4) float32, Xw (M, 3) float32, erase (E bool), the job's
    RESULT_DTYPE record)."""
    jobs, a = make_batch([dict(Tcw=Tcw, fixed=fixed, cam=cam, Xw=Xw, pose_idx=pose_idx, point_idx=point_idx, obs=obs,
                               inv_sigma2=inv_sigma2, n_local=n_local)])
    res, T, X, er = local_ba_batch(jobs, *(a[n] for n, *_ in INPUTS))
    return T.reshape(-1, 4, 4).copy(), X, er.astype(bool), res[0]


# ---- one neighbourhood over the whole chip, with the stop flag (include/orbgpu_localba_chip.h) ----

class LocalBAChipResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("rounds", ctypes.c_int), ("n_bad_first", ctypes.c_int),
                ("n_erase", ctypes.c_int), ("stop_poll", ctypes.c_int), ("polls", ctypes.c_int),
                ("lm_iterations", ctypes.c_int * 2), ("lm_rejected", ctypes.c_int * 2), ("stopped", ctypes.c_int * 2),
                ("iterations_applied", ctypes.c_int * 2), ("n_free", ctypes.c_int * 2),
                ("n_active_points", ctypes.c_int * 2)]


CHIP_RESULT_DTYPE = np.dtype([("status", "<i4"), ("rounds", "<i4"), ("n_bad_first", "<i4"), ("n_erase", "<i4"),
                              ("stop_poll", "<i4"), ("polls", "<i4"), ("lm_iterations", "<i4", (2,)),
                              ("lm_rejected", "<i4", (2,)), ("stopped", "<i4", (2,)),
                              ("iterations_applied", "<i4", (2,)), ("n_free", "<i4", (2,)),
                              ("n_active_points", "<i4", (2,))])
assert CHIP_RESULT_DTYPE.itemsize == ctypes.sizeof(LocalBAChipResult) == 72
CHIP_ITERATIONS = (5, 10)  # Optimizer.cpp:760, 813
_CHIP_BOUND = False


def _chip_lib():
    global _CHIP_BOUND
    L = orbgpu.lib()
    if not _CHIP_BOUND:
        i, sz, vp = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
        L.orbgpu_local_ba_chip_workspace_bytes.argtypes = [i, i, i, i]
        L.orbgpu_local_ba_chip_workspace_bytes.restype = sz
        L.orbgpu_local_ba_chip_device.argtypes = [i, i, i, i] + [vp] * 8 + [i, i, vp, i] + [vp] * 5 + [sz, vp]
        L.orbgpu_local_ba_chip.argtypes = [i, i, i, i] + [vp] * 8 + [i, i, vp, i] + [vp] * 5 + [sz]
        _CHIP_BOUND = True
    return L


def chip_workspace_bytes(n_poses: int, n_local: int, n_points: int, n_edges: int) -> int:
    return int(_chip_lib().orbgpu_local_ba_chip_workspace_bytes(n_poses, n_local, n_points, n_edges))


def local_ba_chip(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local, iterations=CHIP_ITERATIONS,
                  stop=None, stop_at_poll=-1):
    """Host form of orbgpu_local_ba_chip: one neighbourhood over the whole chip.  Returns (Tcw (n_local, 4, 4)
    float32, Xw (M, 3) float32, erase (E) uint8, the CHIP_RESULT_DTYPE record).  stop: a globalba.StopFlag,
    or None; stop_at_poll: the replay of a recorded run's stop_poll."""
    _, a = make_batch([dict(Tcw=Tcw, fixed=fixed, cam=cam, Xw=Xw, pose_idx=pose_idx, point_idx=point_idx, obs=obs,
                            inv_sigma2=inv_sigma2, n_local=n_local)])
    tp, tm, te, nl = len(a["Tcw"]), len(a["Xw"]), len(a["obs"]), int(n_local)
    if not (len(a["fixed"]) == len(a["cam"]) == tp and len(a["edge_pose"]) == len(a["edge_point"]) == te
            and len(a["inv_sigma2"]) == te):
        raise ValueError("pose arrays need one row per pose, edge arrays one row per edge")
    T, X, er = np.zeros((max(nl, 0), 16), np.float32), np.zeros((tm, 3), np.float32), np.zeros(te, np.uint8)
    res = np.zeros(1, CHIP_RESULT_DTYPE)
    orbgpu._check(_chip_lib().orbgpu_local_ba_chip(
        tp, nl, tm, te, *(a[n].ctypes.data for n, *_ in INPUTS), int(iterations[0]), int(iterations[1]),
        stop.ptr if stop is not None else None, int(stop_at_poll), T.ctypes.data, X.ctypes.data, er.ctypes.data,
        res.ctypes.data, None, 0), "orbgpu_local_ba_chip")
    return T.reshape(-1, 4, 4), X, er, res[0]


def local_ba_chip_device(Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2, n_local, Tcw_out, Xw_out, erase,
                         workspace, iterations=CHIP_ITERATIONS, stream=None, stop=None, stop_at_poll=-1,
                         n_poses=None, n_points=None, n_edges=None):
    """Device form on torch tensors of one GPU, in local_ba_batch_device's shapes for one job: Tcw_out float32
    (>= n_local, 16), Xw_out float32 (M, 3), erase uint8 (E); workspace: a contiguous uint8 tensor of at least
    chip_workspace_bytes(P, n_local, M, E) bytes.  n_poses / n_points / n_edges: the job's counts when the
    tensors are larger than the job (their leading rows are the job's).  Synchronous; its launches go to
    `stream`.  Returns the CHIP_RESULT_DTYPE record."""
    tp = Tcw.shape[0] if n_poses is None else int(n_poses)
    tm = Xw.shape[0] if n_points is None else int(n_points)
    te = obs.shape[0] if n_edges is None else int(n_edges)
    for t, rows, cols, name in ((Tcw, tp, 12, "Tcw"), (fixed, tp, 0, "fixed"), (cam, tp, 5, "cam"), (Xw, tm, 3, "Xw"),
                                (edge_pose, te, 0, "edge_pose"), (edge_point, te, 0, "edge_point"), (obs, te, 3, "obs"),
                                (inv_sigma2, te, 0, "inv_sigma2"), (Tcw_out, int(n_local), 16, "Tcw_out"),
                                (Xw_out, tm, 3, "Xw_out"), (erase, te, 0, "erase")):
        if t.shape[0] < rows or tuple(t.shape[1:]) != ((cols,) if cols else ()) or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor of at least {rows} rows of {cols or 1}")
    if workspace.dim() != 1 or not workspace.is_contiguous() or workspace.element_size() != 1:
        raise ValueError("workspace: expected a contiguous one-dimensional uint8 tensor")
    res = np.zeros(1, CHIP_RESULT_DTYPE)
    p = orbgpu._ptr
    orbgpu._check(_chip_lib().orbgpu_local_ba_chip_device(
        tp, int(n_local), tm, te, p(Tcw), p(fixed), p(cam), p(Xw), p(edge_pose), p(edge_point), p(obs), p(inv_sigma2),
        int(iterations[0]), int(iterations[1]), stop.ptr if stop is not None else None, int(stop_at_poll), p(Tcw_out),
        p(Xw_out), p(erase), res.ctypes.data, p(workspace), workspace.numel(), orbgpu._stream_ptr(stream)),
        "orbgpu_local_ba_chip_device")
    return res[0]


# ---- against the map mirror: gather, solve, collect on one stream (include/orbgpu_localba_map.h) ----

MAP_OK, MAP_CAPACITY, MAP_BAD_JOB = 0, 2, 3  # ORBGPU_LOCALBA_MAP_*
_vp = ctypes.c_void_p
_MAP_BOUND = False


class MapMirrorBAStruct(ctypes.Structure):
    _fields_ = [("n_covis_all_total", ctypes.c_int), ("pad", ctypes.c_int), ("covis_all_offset", _vp),
                ("n_covis_all", _vp), ("covis_all", _vp), ("kf_first", _vp), ("kf_Tcw", _vp), ("kf_cam", _vp),
                ("kp_obs", _vp), ("kp_inv_sigma2", _vp), ("obs_idx", _vp)]


class GatherJob(ctypes.Structure):
    _fields_ = [("kf", ctypes.c_int), ("pad", ctypes.c_int)]


class GatherResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_local", ctypes.c_int), ("n_fixed", ctypes.c_int),
                ("n_points", ctypes.c_int), ("n_edges", ctypes.c_int), ("n_mono", ctypes.c_int),
                ("n_stereo", ctypes.c_int), ("pad", ctypes.c_int)]


GATHER_RESULT_DTYPE = np.dtype([(name, "<i4") for name, _ in GatherResult._fields_])
assert GATHER_RESULT_DTYPE.itemsize == ctypes.sizeof(GatherResult) == 32 and ctypes.sizeof(GatherJob) == 8

# the lists a write-back needs: (name, which stride counts its entries per job)
LISTS = (("local_kfs", "kf"), ("fixed_kfs", "pose"), ("local_points", "point"), ("edge_kf", "edge"), ("edge_slot", "edge"))


def _map_lib():
    global _MAP_BOUND
    L = orbgpu.lib()
    if not _MAP_BOUND:
        import track
        i = ctypes.c_int
        L.orbgpu_local_ba_gather_workspace_bytes.argtypes = [i, i, i]
        L.orbgpu_local_ba_gather_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_local_ba_gather_batch_device.argtypes = [i, _vp, ctypes.POINTER(track.MapMirrorStruct),
                                                           ctypes.POINTER(MapMirrorBAStruct), i, i, i, i] + [_vp] * 17
        L.orbgpu_local_ba_collect_batch_device.argtypes = [i, _vp, i, i, i] + [_vp] * 11 + [i, i, _vp, _vp, _vp]
        _MAP_BOUND = True
    return L


class MapMirrorBA:
    """What the gather reads beside a track.MapMirror, uploaded from numpy: covis_all (per keyframe the whole
    ordered covisibility list), kf_first (n_kf,), kf_Tcw (n_kf, 12), kf_cam (n_kf, 5), kp_obs / kp_inv_sigma2
    (per keyframe an (n_slots, 3) / (n_slots,) array, parallel to the mirror's slots), obs_idx (per point a
    list parallel to its observations).  The caller keeps it current."""

    def __init__(self, covis_all, kf_first, kf_Tcw, kf_cam, kp_obs, kp_inv_sigma2, obs_idx, device="cuda"):
        import track
        co, cn, cf = track._ragged(covis_all)
        flat = lambda rows, cols: np.concatenate([np.asarray(r, np.float32).reshape(-1, cols) for r in rows] +
                                                 [np.zeros((0, cols), np.float32)])
        host = {"covis_all_offset": (co, np.int32), "n_covis_all": (cn, np.int32), "covis_all": (cf, np.int32),
                "kf_first": (kf_first, np.uint8), "kf_Tcw": (kf_Tcw, np.float32), "kf_cam": (kf_cam, np.float32),
                "kp_obs": (flat(kp_obs, 3), np.float32), "kp_inv_sigma2": (flat(kp_inv_sigma2, 1), np.float32),
                "obs_idx": (track._ragged(obs_idx)[2], np.int32)}
        self.t = {name: track._up(a, dt, device) for name, (a, dt) in host.items()}
        c = self.c = MapMirrorBAStruct()
        c.n_covis_all_total = len(cf)
        for name, t in self.t.items():
            setattr(c, name, track._ptr(t))


def gather_workspace_bytes(n: int, n_kf: int, n_pt: int) -> int:
    return int(_map_lib().orbgpu_local_ba_gather_workspace_bytes(n, n_kf, n_pt))


class MapLocalBA:
    """LocalBundleAdjustment of n keyframes against a track.MapMirror and a MapMirrorBA as three calls on one
    stream: gather(), solve() (orbgpu_local_ba_batch_device, unchanged) and collect().  Job k owns the rows
    [k * stride, (k + 1) * stride) of every buffer in `t` (torch tensors), so nothing is downloaded between
    the calls.  kfs: pKF's index per job."""

    def __init__(self, mirror, mirror_ba, kfs, kf_stride, pose_stride, point_stride, edge_stride, device="cuda"):
        import torch
        self.mirror, self.mirror_ba, self.n = mirror, mirror_ba, len(kfs)
        self.strides = dict(kf=int(kf_stride), pose=int(pose_stride), point=int(point_stride), edge=int(edge_stride))
        n, S = max(self.n, 1), self.strides
        jobs = np.zeros((n, 2), np.int32)
        jobs[:self.n, 0] = np.asarray(kfs, np.int32).reshape(-1)
        t = self.t = {"gather_jobs": torch.from_numpy(jobs).to(device)}
        zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
        tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}
        for name, dtype, cols, total in INPUTS + OUTPUTS:
            rows = n * S[{"poses": "pose", "local": "kf", "points": "point", "edges": "edge"}[total]]
            t[name] = zeros((rows, cols) if cols else (rows,), tdt[dtype])
        for name, stride in LISTS:
            t[name] = zeros((n, S[stride]), torch.int32)
        t["to_erase"] = zeros((n, S["edge"], 3), torch.int32)
        t["n_erase"] = zeros((n,), torch.int32)
        t["gather_results"] = zeros((n, 32), torch.uint8)
        t["jobs"] = zeros((n, 32), torch.uint8)
        t["results"] = zeros((n, 32), torch.uint8)
        t["gather_ws"] = zeros((max(gather_workspace_bytes(n, mirror.n_kf, mirror.n_pt), 1),), torch.uint8)
        self._zeros = zeros

    def gather(self, stream=None) -> None:
        t, S, p = self.t, self.strides, orbgpu._ptr
        orbgpu._check(_map_lib().orbgpu_local_ba_gather_batch_device(
            self.n, p(t["gather_jobs"]), ctypes.byref(self.mirror.c), ctypes.byref(self.mirror_ba.c), S["kf"], S["pose"],
            S["point"], S["edge"], p(t["gather_ws"]), p(t["gather_results"]), p(t["jobs"]),
            *(p(t[name]) for name, *_ in INPUTS), *(p(t[name]) for name, _ in LISTS), orbgpu._stream_ptr(stream)),
            "orbgpu_local_ba_gather_batch_device")

    def solve_workspace(self):
        """LBA's workspace, allocated at its first use: it grows with the square of kf_stride"""
        import torch
        if "ws" not in self.t:
            n, S = max(self.n, 1), self.strides
            size = workspace_bytes(n, n * S["pose"], n * S["point"], n * S["edge"], S["kf"])
            self.t["ws"] = self._zeros((max(size, 8),), torch.uint8)
        return self.t["ws"]

    def chip_workspace(self):
        """local_ba_chip_device's workspace for one job of the strides' size, allocated at its first use"""
        import torch
        if "chip_ws" not in self.t:
            S = self.strides
            size = chip_workspace_bytes(S["pose"], S["kf"], S["point"], S["edge"])
            self.t["chip_ws"] = self._zeros((max(size, 8),), torch.uint8)
        return self.t["chip_ws"]

    def _solve_chip(self, stream, stop) -> None:
        """the single job over the whole chip: the gathered job record is read back (one small copy), the
        call runs on the gathered arrays in place and leaves its outputs where collect() reads them;
        chip_result is its record, or None for a job the gather rejected (no call is made)"""
        import contextlib
        import torch
        if self.n != 1:
            raise ValueError("chip=True takes a single job")
        t = self.t
        ws = self.chip_workspace()
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            j = t["jobs"][:1].cpu().numpy().reshape(-1).view(JOB_DTYPE)[0]
        self.chip_result = None
        if min(int(j[k]) for k in ("n_poses", "n_local", "n_points", "n_edges")) < 0:
            return
        po, lo, eo, oo = (int(j[k]) for k in ("pose_offset", "point_offset", "edge_offset", "out_pose_offset"))
        off = {"poses": po, "points": lo, "edges": eo, "local": oo}
        ins = [t[name][off[total]:] for name, _, _, total in INPUTS]
        outs = [t[name][off[total]:] for name, _, _, total in OUTPUTS]
        self.chip_result = local_ba_chip_device(*ins, int(j["n_local"]), *outs, ws, stream=stream, stop=stop,
                                                n_poses=int(j["n_poses"]), n_points=int(j["n_points"]),
                                                n_edges=int(j["n_edges"]))

    def solve(self, stream=None, chip=False, stop=None) -> None:
        """call solve_workspace() first when `stream` is not the current one: the allocation is on the current.
        chip=True (a single job): orbgpu_local_ba_chip_device in place of the batched launch, synchronous,
        with `stop` (a globalba.StopFlag) polled as g2o polls it; call chip_workspace() first likewise"""
        if chip:
            return self._solve_chip(stream, stop)
        t = self.t
        self.solve_workspace()
        local_ba_batch_device(t["jobs"][:self.n], *(t[name] for name, *_ in INPUTS), *(t[name] for name, *_ in OUTPUTS),
                              t["results"][:self.n], t["ws"], self.strides["kf"], stream)

    def collect(self, stream=None, write_mirror=False) -> None:
        """write_mirror: scatter the optimised poses and points into mirror_ba's kf_Tcw and the mirror's pos
        (not for a batch whose jobs share a local keyframe or point)"""
        t, S, p = self.t, self.strides, orbgpu._ptr
        kf_Tcw = p(self.mirror_ba.t["kf_Tcw"]) if write_mirror else None
        pos = p(self.mirror.t["pos"]) if write_mirror else None
        orbgpu._check(_map_lib().orbgpu_local_ba_collect_batch_device(
            self.n, p(t["jobs"]), S["kf"], S["point"], S["edge"], p(t["obs"]), p(t["edge_point"]), p(t["local_kfs"]),
            p(t["local_points"]), p(t["edge_kf"]), p(t["edge_slot"]), p(t["erase"]), p(t["Tcw_out"]), p(t["Xw_out"]),
            p(t["to_erase"]), p(t["n_erase"]), self.mirror.n_kf, self.mirror.n_pt, kf_Tcw, pos,
            orbgpu._stream_ptr(stream)), "orbgpu_local_ba_collect_batch_device")

    def run(self, stream=None, write_mirror=False) -> None:
        self.gather(stream)
        self.solve(stream)
        self.collect(stream, write_mirror)

    def host(self, name) -> np.ndarray:
        """a buffer downloaded; the three struct tables as record arrays"""
        a = self.t[name].cpu().numpy()
        dt = {"gather_results": GATHER_RESULT_DTYPE, "jobs": JOB_DTYPE, "results": RESULT_DTYPE}.get(name)
        return a.reshape(-1).view(dt) if dt is not None else a
