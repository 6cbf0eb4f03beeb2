"""Host-side mirror of the Sim3 refinement over the C ABI in
include/orbgpu_sim3opt.h (Optimizer::OptimizeSim3, src/Optimizer.cpp:
1229-1433; the kernel is csrc/sim3opt.hip).

* ``optimize_sim3_batch`` -- the host form on numpy arrays: many loop
  candidates in one launch.
* ``optimize_sim3_batch_device`` -- the device form on torch tensors,
  asynchronous on a stream.
* ``optimize_sim3`` -- one candidate: (n_in, (q12, t12, s12), T12, removed).
"""
from __future__ import annotations

import ctypes

import numpy as np

import orbgpu


class Sim3OptJob(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("offset", ctypes.c_int), ("q12", ctypes.c_double * 4),
                ("t12", ctypes.c_double * 3), ("s12", ctypes.c_double), ("K1", ctypes.c_float * 4),
                ("K2", ctypes.c_float * 4), ("th2", ctypes.c_float), ("fix_scale", ctypes.c_int)]


class Sim3OptResult(ctypes.Structure):
    _fields_ = [("n_in", ctypes.c_int), ("rounds", ctypes.c_int), ("n_bad_first", ctypes.c_int),
                ("lm_iterations", ctypes.c_int * 2), ("lm_rejected", ctypes.c_int * 2), ("pad", ctypes.c_int),
                ("q12", ctypes.c_double * 4), ("t12", ctypes.c_double * 3), ("s12", ctypes.c_double),
                ("T12", ctypes.c_float * 16)]


JOB_DTYPE = np.dtype([("n", "<i4"), ("offset", "<i4"), ("q12", "<f8", (4,)), ("t12", "<f8", (3,)), ("s12", "<f8"),
                      ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("th2", "<f4"), ("fix_scale", "<i4")])
RESULT_DTYPE = np.dtype([("n_in", "<i4"), ("rounds", "<i4"), ("n_bad_first", "<i4"), ("lm_iterations", "<i4", (2,)),
                         ("lm_rejected", "<i4", (2,)), ("pad", "<i4"), ("q12", "<f8", (4,)), ("t12", "<f8", (3,)),
                         ("s12", "<f8"), ("T12", "<f4", (16,))])
assert JOB_DTYPE.itemsize == ctypes.sizeof(Sim3OptJob) == 112
assert RESULT_DTYPE.itemsize == ctypes.sizeof(Sim3OptResult) == 160

# the batch arrays: (name, floats per correspondence)
ARRAYS = (("P1c", 3), ("P2c", 3), ("obs1", 2), ("obs2", 2), ("inv_sigma2_1", 1), ("inv_sigma2_2", 1))


def make_jobs(candidates) -> np.ndarray:
    """JOB_DTYPE array of `candidates`: an iterable of (n, offset, q12 (x, y,
    z, w), t12, s12, K1, K2 (fx, fy, cx, cy), th2, fix_scale)."""
    candidates = list(candidates)
    jobs = np.zeros(len(candidates), JOB_DTYPE)
    for j, (n, offset, q12, t12, s12, K1, K2, th2, fix_scale) in zip(jobs, candidates):
        j["n"], j["offset"] = n, offset
        j["q12"], j["t12"], j["s12"] = q12, t12, s12
        j["K1"], j["K2"] = K1, K2
        j["th2"], j["fix_scale"] = th2, int(bool(fix_scale))
    return jobs


def optimize_sim3_batch(jobs, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, removed=None):
    """Host form of orbgpu_optimize_sim3_batch.  jobs: JOB_DTYPE array (or a
    ctypes array of Sim3OptJob); P1c, P2c (total, 3), obs1, obs2 (total, 2),
    inv_sigma2_1, inv_sigma2_2 (total).  Returns (results as a RESULT_DTYPE
    array, removed uint8 (total)); `removed`, when given, is updated in place
    (bytes outside every job's range keep their values)."""
    if not isinstance(jobs, np.ndarray):
        jobs = np.frombuffer(bytes(jobs), JOB_DTYPE)
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    arrays = [np.ascontiguousarray(a, np.float32).reshape(-1, w)
              for a, (_, w) in zip((P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2), ARRAYS)]
    total = len(arrays[0])
    if any(len(a) != total for a in arrays):
        raise ValueError("the six correspondence arrays must have one row per correspondence")
    if removed is None:
        removed = np.zeros(total, np.uint8)
    if removed.dtype != np.uint8 or removed.shape != (total,) or not removed.flags.c_contiguous:
        raise ValueError("removed must be a contiguous uint8 array with one byte per correspondence")
    res = np.zeros(len(jobs), RESULT_DTYPE)
    orbgpu._check(orbgpu.lib().orbgpu_optimize_sim3_batch(
        len(jobs), jobs.ctypes.data, total, *(a.ctypes.data for a in arrays), res.ctypes.data, removed.ctypes.data),
        "orbgpu_optimize_sim3_batch")
    return res, removed


def optimize_sim3_batch_device(jobs, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, results, removed,
                               stream=None) -> None:
    """Device form on torch tensors of one GPU: jobs uint8 (B, 112) (JOB_DTYPE
    bytes), P1c / P2c float32 (total, 3), obs1 / obs2 float32 (total, 2),
    inv_sigma2_1 / inv_sigma2_2 float32 (total), results uint8 (B, 160)
    (RESULT_DTYPE bytes), removed uint8 (total).  Asynchronous on `stream`
    (default: the null stream)."""
    B, total = jobs.shape[0], P1c.shape[0]
    for t, shape, name in ((jobs, (B, JOB_DTYPE.itemsize), "jobs"), (P1c, (total, 3), "P1c"), (P2c, (total, 3), "P2c"),
                           (obs1, (total, 2), "obs1"), (obs2, (total, 2), "obs2"),
                           (inv_sigma2_1, (total,), "inv_sigma2_1"), (inv_sigma2_2, (total,), "inv_sigma2_2"),
                           (results, (B, RESULT_DTYPE.itemsize), "results"), (removed, (total,), "removed")):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous tensor of shape {shape}")
    orbgpu._check(orbgpu.lib().orbgpu_optimize_sim3_batch_device(
        B, orbgpu._ptr(jobs), total, orbgpu._ptr(P1c), orbgpu._ptr(P2c), orbgpu._ptr(obs1), orbgpu._ptr(obs2),
        orbgpu._ptr(inv_sigma2_1), orbgpu._ptr(inv_sigma2_2), orbgpu._ptr(results), orbgpu._ptr(removed),
        orbgpu._stream_ptr(stream)), "orbgpu_optimize_sim3_batch_device")


def optimize_sim3(q12, t12, s12, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale):
    """Optimizer::OptimizeSim3 of one candidate.  Returns (n_in, (q12, t12,
    s12) in float64 -- the input's values when the reference does not write
    g2oS12 --, T12 (4x4 float32), removed (n bool))."""
    P1c = np.ascontiguousarray(P1c, np.float32).reshape(-1, 3)
    jobs = make_jobs([(len(P1c), 0, q12, t12, s12, K1, K2, th2, fix_scale)])
    res, removed = optimize_sim3_batch(jobs, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2)
    r = res[0]
    return (int(r["n_in"]), (r["q12"].copy(), r["t12"].copy(), float(r["s12"])), r["T12"].reshape(4, 4).copy(),
            removed.astype(bool))
