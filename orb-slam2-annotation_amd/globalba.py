"""Host-side mirror of the global bundle adjustment over the C ABI in
include/orbgpu_globalba.h (Optimizer::BundleAdjustment, src/Optimizer.cpp:
72-269; the kernels are csrc/globalba.hip).

* ``bundle_adjustment`` -- the host form on numpy arrays: one problem.
* ``bundle_adjustment_device`` -- the device form on torch tensors with a
  caller-provided workspace; synchronous, its launches go to ``stream``.
* ``StopFlag`` -- a byte of host memory that another thread may set.
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu


class BAResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("iterations", ctypes.c_int), ("rejected", ctypes.c_int),
                ("stopped", ctypes.c_int), ("iterations_applied", ctypes.c_int), ("n_free", ctypes.c_int),
                ("n_active_points", ctypes.c_int), ("pad", ctypes.c_int), ("first_chi2", ctypes.c_double),
                ("last_chi2", ctypes.c_double), ("last_lambda", ctypes.c_double)]


RESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("rejected", "<i4"), ("stopped", "<i4"),
                         ("iterations_applied", "<i4"), ("n_free", "<i4"), ("n_active_points", "<i4"), ("pad", "<i4"),
                         ("first_chi2", "<f8"), ("last_chi2", "<f8"), ("last_lambda", "<f8")])
assert RESULT_DTYPE.itemsize == ctypes.sizeof(BAResult) == 56

# the arrays in the order of the C ABI: (name, dtype, columns, which count its rows are)
INPUTS = (("Tcw", np.float32, 12, "poses"), ("fixed", np.uint8, 0, "poses"), ("cam", np.float32, 5, "poses"),
          ("Xw", np.float32, 3, "points"), ("edge_pose", np.int32, 0, "edges"), ("edge_point", np.int32, 0, "edges"),
          ("obs", np.float32, 3, "edges"), ("inv_sigma2", np.float32, 0, "edges"))
OUTPUTS = (("Tcw_out", np.float32, 16, "poses"), ("Xw_out", np.float32, 3, "points"))

_vp = ctypes.c_void_p
_BOUND = False


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        i, sz = ctypes.c_int, ctypes.c_size_t
        L.orbgpu_bundle_adjustment_workspace_bytes.argtypes = [i, i, i]
        L.orbgpu_bundle_adjustment_workspace_bytes.restype = sz
        L.orbgpu_bundle_adjustment_device.argtypes = [i, i, i] + [_vp] * 8 + [i, i, _vp, _vp, _vp, _vp, _vp, sz, _vp]
        L.orbgpu_bundle_adjustment.argtypes = [i, i, i] + [_vp] * 8 + [i, i, _vp, _vp, _vp, _vp, _vp, sz]
        _BOUND = True
    return L


class StopFlag:
    """*pbStopFlag: one byte of host memory"""

    def __init__(self, value: bool = False):
        self.byte = ctypes.c_uint8(1 if value else 0)

    def set(self, value: bool = True) -> None:
        self.byte.value = 1 if value else 0

    @property
    def ptr(self) -> int:
        return ctypes.addressof(self.byte)


def workspace_bytes(n_poses: int, n_points: int, n_edges: int) -> int:
    return int(_lib().orbgpu_bundle_adjustment_workspace_bytes(n_poses, n_points, n_edges))


def pack(Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2):
    """the arrays of INPUTS, contiguous, in the ABI's types; Tcw may be (P, 3x4 or 4x4)"""
    T = np.asarray(Tcw, np.float32)
    T = T.reshape(len(T), -1, 4)[:, :3].reshape(len(T), 12) if len(T) else np.zeros((0, 12), np.float32)
    a = {"Tcw": np.ascontiguousarray(T)}
    for (name, dtype, cols, _), val in zip(INPUTS[1:], (fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2)):
        a[name] = np.ascontiguousarray(val, dtype).reshape((-1, cols) if cols else (-1,))
    tp, te = len(a["Tcw"]), len(a["obs"])
    if not (len(a["fixed"]) == len(a["cam"]) == tp and len(a["edge_pose"]) == len(a["edge_point"]) == te
            and len(a["inv_sigma2"]) == te):
        raise ValueError("pose arrays need one row per pose, edge arrays one row per edge")
    return a


def bundle_adjustment(Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2, n_iterations, robust, stop=None):
    """Host form of orbgpu_bundle_adjustment.  Returns (Tcw (P, 4, 4) float32, Xw (M, 3) float32, the
    RESULT_DTYPE record).  stop: a StopFlag, or None."""
    a = pack(Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2)
    tp, tm, te = len(a["Tcw"]), len(a["Xw"]), len(a["obs"])
    T, X = np.zeros((tp, 16), np.float32), np.zeros((tm, 3), np.float32)
    res = np.zeros(1, RESULT_DTYPE)
    orbgpu._check(_lib().orbgpu_bundle_adjustment(
        tp, tm, te, *(a[n].ctypes.data for n, *_ in INPUTS), int(n_iterations), int(bool(robust)),
        stop.ptr if stop is not None else None, T.ctypes.data, X.ctypes.data, res.ctypes.data, None, 0),
        "orbgpu_bundle_adjustment")
    return T.reshape(-1, 4, 4), X, res[0]


def bundle_adjustment_device(Tcw, fixed, cam, Xw, edge_pose, edge_point, obs, inv_sigma2, n_iterations, robust, Tcw_out,
                             Xw_out, workspace, stream=None, stop=None):
    """Device form on torch tensors of one GPU: Tcw float32 (P, 12), fixed uint8 (P), cam float32 (P, 5), Xw
    float32 (M, 3), edge_pose / edge_point int32 (E), obs float32 (E, 3), inv_sigma2 float32 (E); Tcw_out
    float32 (P, 16), Xw_out float32 (M, 3); workspace: a contiguous uint8 tensor of at least
    workspace_bytes(P, M, E) bytes.  Synchronous; returns the RESULT_DTYPE record."""
    tp, tm, te = Tcw.shape[0], Xw.shape[0], obs.shape[0]
    for t, shape, name in ((Tcw, (tp, 12), "Tcw"), (fixed, (tp,), "fixed"), (cam, (tp, 5), "cam"), (Xw, (tm, 3), "Xw"),
                           (edge_pose, (te,), "edge_pose"), (edge_point, (te,), "edge_point"), (obs, (te, 3), "obs"),
                           (inv_sigma2, (te,), "inv_sigma2"), (Tcw_out, (tp, 16), "Tcw_out"), (Xw_out, (tm, 3), "Xw_out")):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor of shape {shape}")
    if workspace.dim() != 1 or not workspace.is_contiguous() or workspace.element_size() != 1:
        raise ValueError("workspace: expected a contiguous one-dimensional uint8 tensor")
    res = np.zeros(1, RESULT_DTYPE)
    p = orbgpu._ptr
    orbgpu._check(_lib().orbgpu_bundle_adjustment_device(
        tp, tm, te, p(Tcw), p(fixed), p(cam), p(Xw), p(edge_pose), p(edge_point), p(obs), p(inv_sigma2),
        int(n_iterations), int(bool(robust)), stop.ptr if stop is not None else None, p(Tcw_out), p(Xw_out),
        res.ctypes.data, p(workspace), workspace.numel(), orbgpu._stream_ptr(stream)),
        "orbgpu_bundle_adjustment_device")
    return res[0]
