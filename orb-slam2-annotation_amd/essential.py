"""Host-side mirror of the essential-graph optimisation over the C ABI in
include/orbgpu_essential.h (Optimizer::OptimizeEssentialGraph, src/Optimizer.cpp:
905-1200; the kernels are csrc/essential.hip).

* ``optimize_essential_graph`` -- the host form on numpy arrays: one graph.
* ``optimize_essential_graph_device`` -- the device form on torch tensors with a
  caller-provided workspace; synchronous, its launches go to ``stream``.
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu


class EGResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("iterations", ctypes.c_int), ("rejected", ctypes.c_int),
                ("n_free", ctypes.c_int), ("n_active_edges", ctypes.c_int), ("pad", ctypes.c_int * 3),
                ("first_chi2", ctypes.c_double), ("last_chi2", ctypes.c_double), ("last_lambda", ctypes.c_double)]


RESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("rejected", "<i4"), ("n_free", "<i4"),
                         ("n_active_edges", "<i4"), ("pad", "<i4", (3,)), ("first_chi2", "<f8"), ("last_chi2", "<f8"),
                         ("last_lambda", "<f8")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(EGResult) == 56

# the arrays in the order of the C ABI: (name, dtype, columns, which count its rows are)
INPUTS = (("Tcw", np.float32, 12, "kf"), ("has_corrected", np.uint8, 0, "kf"), ("Scorrected", np.float64, 8, "kf"),
          ("has_noncorrected", np.uint8, 0, "kf"), ("Snoncorrected", np.float64, 8, "kf"), ("fixed", np.uint8, 0, "kf"),
          ("edge_i", np.int32, 0, "edges"), ("edge_j", np.int32, 0, "edges"), ("edge_kind", np.uint8, 0, "edges"),
          ("Xw", np.float32, 3, "points"), ("point_ref", np.int32, 0, "points"))
OUTPUTS = (("Scw_out", np.float64, 8, "kf"), ("Tcw_out", np.float32, 16, "kf"), ("Xw_out", np.float32, 3, "points"))

_vp = ctypes.c_void_p
_BOUND = False


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        i, sz = ctypes.c_int, ctypes.c_size_t
        L.orbgpu_essential_graph_workspace_bytes.argtypes = [i, i, i]
        L.orbgpu_essential_graph_workspace_bytes.restype = sz
        L.orbgpu_optimize_essential_graph_device.argtypes = [i, i, i] + [_vp] * 11 + [i, i] + [_vp] * 5 + [sz, _vp]
        L.orbgpu_optimize_essential_graph.argtypes = [i, i, i] + [_vp] * 11 + [i, i] + [_vp] * 5 + [sz]
        _BOUND = True
    return L


def workspace_bytes(n_kf: int, n_edges: int, n_points: int) -> int:
    return int(_lib().orbgpu_essential_graph_workspace_bytes(n_kf, n_edges, n_points))


def pack(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j, edge_kind, Xw,
         point_ref):
    """the arrays of INPUTS, contiguous, in the ABI's types; Tcw may be (N, 3x4 or 4x4)"""
    T = np.asarray(Tcw, np.float32)
    T = T.reshape(len(T), -1, 4)[:, :3].reshape(len(T), 12) if len(T) else np.zeros((0, 12), np.float32)
    a = {"Tcw": np.ascontiguousarray(T)}
    vals = (has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j, edge_kind, Xw, point_ref)
    for (name, dtype, cols, _), val in zip(INPUTS[1:], vals):
        a[name] = np.ascontiguousarray(val, dtype).reshape((-1, cols) if cols else (-1,))
    counts = {"kf": len(a["Tcw"]), "edges": len(a["edge_i"]), "points": len(a["Xw"])}
    for name, _, _, which in INPUTS:
        if len(a[name]) != counts[which]:
            raise ValueError(f"{name}: expected one row per {which} entry ({counts[which]}), got {len(a[name])}")
    return a


def optimize_essential_graph(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j,
                             edge_kind, Xw, point_ref, fix_scale, n_iterations=20):
    """Host form of orbgpu_optimize_essential_graph.  Returns (Scw (N, 8) float64, Tcw (N, 4, 4) float32,
    Xw (M, 3) float32, the RESULT_DTYPE record)."""
    a = pack(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j, edge_kind, Xw,
             point_ref)
    tn, te, tm = len(a["Tcw"]), len(a["edge_i"]), len(a["Xw"])
    S, T, X = np.zeros((tn, 8)), np.zeros((tn, 16), np.float32), np.zeros((tm, 3), np.float32)
    res = np.zeros(1, RESULT_DTYPE)
    orbgpu._check(_lib().orbgpu_optimize_essential_graph(
        tn, te, tm, *(a[n].ctypes.data for n, *_ in INPUTS), int(bool(fix_scale)), int(n_iterations), S.ctypes.data,
        T.ctypes.data, X.ctypes.data, res.ctypes.data, None, 0), "orbgpu_optimize_essential_graph")
    return S, T.reshape(-1, 4, 4), X, res[0]


def optimize_essential_graph_device(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i,
                                    edge_j, edge_kind, Xw, point_ref, fix_scale, n_iterations, Scw_out, Tcw_out,
                                    Xw_out, workspace, stream=None):
    """Device form on torch tensors of one GPU, shaped and typed as INPUTS and OUTPUTS list them;
    workspace: a contiguous uint8 tensor of at least workspace_bytes(N, E, M) bytes.  Synchronous; returns
    the RESULT_DTYPE record."""
    tensors = (Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j, edge_kind, Xw,
               point_ref, Scw_out, Tcw_out, Xw_out)
    counts = {"kf": Tcw.shape[0], "edges": edge_i.shape[0], "points": Xw.shape[0]}
    for t, (name, _, cols, which) in zip(tensors, INPUTS + OUTPUTS):
        shape = (counts[which], cols) if cols else (counts[which],)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor of shape {shape}")
    if workspace.dim() != 1 or not workspace.is_contiguous() or workspace.element_size() != 1:
        raise ValueError("workspace: expected a contiguous one-dimensional uint8 tensor")
    res = np.zeros(1, RESULT_DTYPE)
    p = orbgpu._ptr
    orbgpu._check(_lib().orbgpu_optimize_essential_graph_device(
        counts["kf"], counts["edges"], counts["points"], *(p(t) for t in tensors[:11]), int(bool(fix_scale)),
        int(n_iterations), *(p(t) for t in tensors[11:]), res.ctypes.data, p(workspace), workspace.numel(),
        orbgpu._stream_ptr(stream)), "orbgpu_optimize_essential_graph_device")
    return res[0]
