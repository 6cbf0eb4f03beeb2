"""Host-side mirror of the motion-only pose optimisation over the C ABI in
include/orbgpu_poseopt.h (Optimizer::PoseOptimization, src/Optimizer.cpp:
291-513; the kernel is csrc/poseopt.hip).

* ``pose_optimization_batch`` -- the host form on numpy arrays: many frames
  (all relocalisation candidates, a batch of tracked frames) in one launch.
* ``pose_optimization_batch_device`` -- the device form on torch tensors,
  asynchronous on a stream.
* ``pose_optimization`` -- one frame: (Tcw, outlier, n_good).
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu


class PoseOptJob(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("offset", ctypes.c_int), ("Tcw0", ctypes.c_float * 12),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("bf", ctypes.c_float), ("pad", ctypes.c_int)]


class PoseOptResult(ctypes.Structure):
    _fields_ = [("n_good", ctypes.c_int), ("rounds", ctypes.c_int), ("lm_iterations", ctypes.c_int * 4),
                ("lm_rejected", ctypes.c_int * 4), ("Tcw", ctypes.c_float * 16)]


JOB_DTYPE = np.dtype([("n", "<i4"), ("offset", "<i4"), ("Tcw0", "<f4", (12,)), ("fx", "<f4"), ("fy", "<f4"),
                      ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4"), ("pad", "<i4")])
RESULT_DTYPE = np.dtype([("n_good", "<i4"), ("rounds", "<i4"), ("lm_iterations", "<i4", (4,)),
                         ("lm_rejected", "<i4", (4,)), ("Tcw", "<f4", (16,))])
assert JOB_DTYPE.itemsize == ctypes.sizeof(PoseOptJob) == 80
assert RESULT_DTYPE.itemsize == ctypes.sizeof(PoseOptResult) == 104


def make_jobs(frames) -> np.ndarray:
    """JOB_DTYPE array of `frames`: an iterable of (n, offset, Tcw0 (3x4 or
    4x4), (fx, fy, cx, cy), bf)."""
    frames = list(frames)
    jobs = np.zeros(len(frames), JOB_DTYPE)
    for j, (n, offset, Tcw0, K, bf) in zip(jobs, frames):
        j["n"], j["offset"] = n, offset
        j["Tcw0"] = np.asarray(Tcw0, np.float32)[:3].reshape(12)
        j["fx"], j["fy"], j["cx"], j["cy"] = K
        j["bf"] = bf
    return jobs


def pose_optimization_batch(jobs, Xw, obs, inv_sigma2, outlier=None):
    """Host form of orbgpu_pose_optimization_batch.  jobs: JOB_DTYPE array (or
    a ctypes array of PoseOptJob); Xw (total, 3), obs (total, 3) = (u, v,
    uRight; uRight < 0: monocular), inv_sigma2 (total).  Returns (results as a
    RESULT_DTYPE array, outlier uint8 (total)); `outlier`, when given, is
    updated in place (bytes outside every job's range keep their values)."""
    if not isinstance(jobs, np.ndarray):
        jobs = np.frombuffer(bytes(jobs), JOB_DTYPE)
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
    total = len(Xw)
    if len(obs) != total or len(w) != total:
        raise ValueError("Xw, obs and inv_sigma2 must have one row per observation")
    if outlier is None:
        outlier = np.zeros(total, np.uint8)
    if outlier.dtype != np.uint8 or outlier.shape != (total,) or not outlier.flags.c_contiguous:
        raise ValueError("outlier must be a contiguous uint8 array with one byte per observation")
    res = np.zeros(len(jobs), RESULT_DTYPE)
    orbgpu._check(orbgpu.lib().orbgpu_pose_optimization_batch(
        len(jobs), jobs.ctypes.data, total, Xw.ctypes.data, obs.ctypes.data, w.ctypes.data, res.ctypes.data,
        outlier.ctypes.data), "orbgpu_pose_optimization_batch")
    return res, outlier


def pose_optimization_batch_device(jobs, Xw, obs, inv_sigma2, results, outlier, stream=None) -> None:
    """Device form on torch tensors of one GPU: jobs uint8 (B, 80) (JOB_DTYPE
    bytes), Xw / obs float32 (total, 3), inv_sigma2 float32 (total), results
    uint8 (B, 104) (RESULT_DTYPE bytes), outlier uint8 (total).  Asynchronous
    on `stream` (default: the null stream)."""
    B, total = jobs.shape[0], Xw.shape[0]
    for t, shape, name in ((jobs, (B, JOB_DTYPE.itemsize), "jobs"), (Xw, (total, 3), "Xw"), (obs, (total, 3), "obs"),
                           (inv_sigma2, (total,), "inv_sigma2"), (results, (B, RESULT_DTYPE.itemsize), "results"),
                           (outlier, (total,), "outlier")):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor of shape {shape}")
    orbgpu._check(orbgpu.lib().orbgpu_pose_optimization_batch_device(
        B, orbgpu._ptr(jobs), total, orbgpu._ptr(Xw), orbgpu._ptr(obs), orbgpu._ptr(inv_sigma2),
        orbgpu._ptr(results), orbgpu._ptr(outlier), orbgpu._stream_ptr(stream)),
        "orbgpu_pose_optimization_batch_device")


def pose_optimization(Tcw, Xw, obs, inv_sigma2, K, bf):
    """Optimizer::PoseOptimization of one frame: Tcw = pFrame->mTcw, one row of
    Xw / obs / inv_sigma2 per keypoint with a MapPoint.  Returns (Tcw (4x4
    float32), outlier (n bool), n_good)."""
    Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    res, out = pose_optimization_batch(make_jobs([(len(Xw), 0, Tcw, K, bf)]), Xw, obs, inv_sigma2)
    return res["Tcw"][0].reshape(4, 4).copy(), out.astype(bool), int(res["n_good"][0])
