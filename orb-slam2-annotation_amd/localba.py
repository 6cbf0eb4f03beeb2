"""Host-side mirror of the local bundle adjustment over the C ABI in
include/orbgpu_localba.h (Optimizer::LocalBundleAdjustment, src/Optimizer.cpp:
536-885; the kernel is csrc/localba.hip).

* ``local_ba_batch`` -- the host form on numpy arrays: many keyframe
  neighbourhoods in one launch.
* ``local_ba_batch_device`` -- the device form on torch tensors, asynchronous
  on a stream, with a caller-provided workspace.
* ``local_bundle_adjustment`` -- one neighbourhood: (Tcw of the local poses,
  Xw, erase, result).
* ``make_jobs`` / ``make_batch`` -- job records, and the concatenated arrays of
  a list of problems.
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
