"""Host-side mirror of Tracking's per-frame chain over the C ABI in
include/orbgpu_track.h (csrc/track.hip).

* ``PointTable`` -- one frame's MapPoint table (flags, positions, descriptors,
  ...) resident in HBM: the last frame's slots or the reference keyframe's for
  the initial pose, the local map followed by the frame-held extras for the
  local-map call.
* ``TrackStep`` -- a batch of frames (a ``reloc.Frames``) taken through
  ``initial`` (TrackWithMotionModel / TrackReferenceKeyFrame,
  src/Tracking.cpp:1126-1198, :977-1025) and ``local_map`` (SearchLocalPoints +
  TrackLocalMap, :1496-1562, :1210-1264).  UpdateLocalMap, between the two, is
  the caller's; ``local_map`` can read the pose ``initial`` left in place.
* ``update_last_frame`` -- UpdateLastFrame's visual-odometry points
  (:1053-1113) for stereo / RGB-D streams.

Everything runs on the GPU; there is no host fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

import bow
import loop
import orbgpu
import poseopt
import proj
import reloc

_BOUND = False

MOTION, REFERENCE = 0, 1
OK, FEW_MATCHES, LOST, CAPACITY, BAD_JOB = range(5)
INITIAL_ROWS, LOCAL_ROWS = 2, 3
ROW_BEFORE_CULL, ROW_AFTER_CULL = 0, 1
ROW_SEARCHED, ROW_FINAL, ROW_OUTLIER = 0, 1, 2
PT_SEEN, PT_IN_VIEW = 1, 2
LAST_SEEN = 8  # ORBGPU_PT_LAST_SEEN: a local_map table flag beside proj.VALID / proj.HAS_OBS
vp = ctypes.c_void_p


class TrackInitialJob(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("frame", ctypes.c_int), ("mono", ctypes.c_int),
                ("only_tracking", ctypes.c_int), ("th", ctypes.c_float), ("pad", ctypes.c_int * 3),
                ("Tcw_init", ctypes.c_float * 16), ("last_Tcw", ctypes.c_float * 16), ("points", proj.Points),
                ("bow_row", vp), ("bow_nmatches", vp)]


class TrackInitialResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("searches", ctypes.c_int), ("nsearch", ctypes.c_int * 2),
                ("nmatches", ctypes.c_int), ("nmatches_map", ctypes.c_int), ("vo", ctypes.c_int),
                ("pad", ctypes.c_int), ("opt", poseopt.PoseOptResult), ("Tcw", ctypes.c_float * 16)]


class TrackLocalJob(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_int), ("n_local", ctypes.c_int), ("stereo", ctypes.c_int),
                ("only_tracking", ctypes.c_int), ("recently_relocalised", ctypes.c_int), ("th", ctypes.c_float),
                ("Tcw", vp), ("frame_mp", vp), ("points", proj.Points)]


class TrackLocalResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_to_match", ctypes.c_int), ("nsearch", ctypes.c_int),
                ("n_inliers", ctypes.c_int), ("opt", poseopt.PoseOptResult), ("Tcw", ctypes.c_float * 16)]


class UpdateLastFrameJob(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("th_depth", ctypes.c_float), ("depth", vp), ("kps_un", vp), ("frame_desc", vp),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("invfx", ctypes.c_float), ("invfy", ctypes.c_float), ("Rwc", ctypes.c_float * 9),
                ("Ow", ctypes.c_float * 3), ("flags", vp), ("pos", vp), ("desc", vp)]


class UpdateLastFrameResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_created", ctypes.c_int), ("n_pos", ctypes.c_int),
                ("n_visited", ctypes.c_int)]


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        i = ctypes.c_int
        L.orbgpu_track_initial_workspace_bytes.argtypes = [i, i]
        L.orbgpu_track_initial_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_track_initial_batch_device.argtypes = [i, vp, i, vp, i, vp, vp, vp, vp]
        L.orbgpu_track_local_workspace_bytes.argtypes = [i, i, i]
        L.orbgpu_track_local_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_track_local_map_batch_device.argtypes = [i, vp, i, vp, i, i, vp, vp, vp, vp, vp]
        L.orbgpu_update_last_frame_batch_device.argtypes = [i, vp, i, vp, vp, vp]
        _BOUND = True
    return L


def _up(a, dtype, device):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(device)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class PointTable:
    """A MapPoint table of n entries in HBM (numpy in): flags (n,) int32 of
    proj.VALID / proj.HAS_OBS, pos (n, 3) f32 and, as the call that reads the
    table needs them, desc (n, 32) u8, normal (n, 3), min_dist, max_dist (n,)
    f32, octave (n,) int32, angle (n,) f32."""

    FIELDS = (("pos", np.float32), ("normal", np.float32), ("desc", np.uint8), ("min_dist", np.float32),
              ("max_dist", np.float32), ("octave", np.int32), ("angle", np.float32))

    def __init__(self, flags, pos, device="cuda", **fields):
        self.n = len(flags)
        self.flags = _up(flags, np.int32, device)
        fields["pos"] = pos
        self.t = {name: _up(fields[name], dt, device) for name, dt in self.FIELDS if fields.get(name) is not None}

    def points(self, n=None) -> proj.Points:
        P = proj.Points()
        P.n = self.n if n is None else int(n)
        P.flags = _ptr(self.flags)
        for name, _ in self.FIELDS:
            setattr(P, name, _ptr(self.t.get(name)))
        return P


def _pose16(T):
    T = np.asarray(T, np.float32)
    if T.size == 12:
        T = np.vstack([T.reshape(3, 4), [[0, 0, 0, 1]]]).astype(np.float32)
    return [float(v) for v in T.reshape(16)]


class TrackStep:
    """The two device calls of an ordinary frame for every frame of `frames`
    (a reloc.Frames: mvKeysUn, descriptors, mvuRight, intrinsics, bounds, the
    scale pyramid and the sigma tables)."""

    def __init__(self, frames: reloc.Frames):
        self.frames, self.device, self.stride = frames, frames.device, frames.stride
        self.n_initial = self.n_local = 0
        self.point_stride = 1

    # ---- 1. TrackWithMotionModel / TrackReferenceKeyFrame -----------------
    def initial(self, jobs, stream=None, n_frames=None):
        """jobs: dicts with mode, frame, table (PointTable), Tcw_init and, in
        motion mode, last_Tcw, th (15 or 7), mono; in reference mode bow_row
        ((stride,) int32 numpy or a device tensor) and bow_nmatches (int or a
        device tensor); optionally only_tracking."""
        import torch
        n, S, dev = len(jobs), self.stride, self.device
        tab = (TrackInitialJob * max(n, 1))()
        held = []
        for J, j in zip(tab, jobs):
            J.mode, J.frame = int(j["mode"]), int(j["frame"])
            J.mono, J.only_tracking = int(j.get("mono", 0)), int(j.get("only_tracking", 0))
            J.th = float(j.get("th", 0.0))
            J.Tcw_init[:] = _pose16(j["Tcw_init"])
            if j.get("last_Tcw") is not None:
                J.last_Tcw[:] = _pose16(j["last_Tcw"])
            held.append(j["table"])
            J.points = j["table"].points()
            row, nm = j.get("bow_row"), j.get("bow_nmatches")
            if row is not None:
                row = row if isinstance(row, torch.Tensor) else _up(row, np.int32, dev)
                nm = nm if isinstance(nm, torch.Tensor) else _up([int(nm)], np.int32, dev)
                held += [row, nm]
                J.bow_row, J.bow_nmatches = row.data_ptr(), nm.data_ptr()
        L = _lib()
        N = max(n, 1)
        self.n_initial = n
        self.d_initial_jobs = bow.to_device_table(tab, dev)
        self.initial_ws = torch.zeros(L.orbgpu_track_initial_workspace_bytes(N, S), dtype=torch.uint8, device=dev)
        self.d_initial_results = torch.zeros(N * ctypes.sizeof(TrackInitialResult), dtype=torch.uint8, device=dev)
        self.d_initial_rows = torch.zeros((N, INITIAL_ROWS, S), dtype=torch.int32, device=dev)
        self._held_initial = held
        self._n_frames_initial = self.frames.n_f if n_frames is None else n_frames
        self.run_initial(stream)

    def run_initial(self, stream=None):
        """the call for the jobs `initial` uploaded last, again (no allocation, no upload)"""
        orbgpu._check(_lib().orbgpu_track_initial_batch_device(
            self.n_initial, self.d_initial_jobs.data_ptr(), self._n_frames_initial, self.frames.d_table.data_ptr(),
            self.stride, self.initial_ws.data_ptr(), self.d_initial_results.data_ptr(), self.d_initial_rows.data_ptr(),
            orbgpu._stream_ptr(stream)), "orbgpu_track_initial_batch_device")

    def initial_results(self):
        return loop._struct_rows(self.d_initial_results, TrackInitialResult, self.n_initial)

    def initial_rows(self):
        """(n, 2, stride) int32 by frame keypoint: mvpMapPoints before and after the cull"""
        return self.d_initial_rows[:self.n_initial].cpu().numpy()

    def initial_pose_ptr(self, k):
        """the device address of job k's resulting mTcw, for local_map's Tcw"""
        return self.d_initial_results.data_ptr() + k * ctypes.sizeof(TrackInitialResult) + TrackInitialResult.Tcw.offset

    # ---- 2. SearchLocalPoints + TrackLocalMap ------------------------------
    def local_map(self, jobs, stream=None, point_stride=None, n_frames=None):
        """jobs: dicts with frame, table (PointTable: the local points, then
        the frame-held extras; LAST_SEEN on the entries call 1 culled),
        n_local, frame_mp ((stride,) int32), Tcw (16 or 12 floats, uploaded; or an int: a device address read when the call
        runs, e.g. initial_pose_ptr(k)), th (1, 3 or 5) and optionally stereo,
        only_tracking, recently_relocalised."""
        import torch
        n, S, dev = len(jobs), self.stride, self.device
        P = int(point_stride) if point_stride is not None else max([j["table"].n for j in jobs] + [1])
        tab = (TrackLocalJob * max(n, 1))()
        held = []
        for J, j in zip(tab, jobs):
            J.frame, J.n_local = int(j["frame"]), int(j["n_local"])
            J.stereo, J.only_tracking = int(j.get("stereo", 0)), int(j.get("only_tracking", 0))
            J.recently_relocalised = int(j.get("recently_relocalised", 0))
            J.th = float(j.get("th", 1.0))
            T = j["Tcw"]
            if isinstance(T, int):
                J.Tcw = T
            elif T is not None:
                t = _up(_pose16(T), np.float32, dev)
                held.append(t)
                J.Tcw = t.data_ptr()
            mp = j.get("frame_mp")
            if mp is not None:
                mp = mp if isinstance(mp, torch.Tensor) else _up(mp, np.int32, dev)
                held.append(mp)
                J.frame_mp = mp.data_ptr()
            held.append(j["table"])
            J.points = j["table"].points()
        L = _lib()
        N = max(n, 1)
        self.n_local, self.point_stride = n, P
        self.d_local_jobs = bow.to_device_table(tab, dev)
        self.local_ws = torch.zeros(L.orbgpu_track_local_workspace_bytes(N, S, P), dtype=torch.uint8, device=dev)
        self.d_local_results = torch.zeros(N * ctypes.sizeof(TrackLocalResult), dtype=torch.uint8, device=dev)
        self.d_local_rows = torch.zeros((N, LOCAL_ROWS, S), dtype=torch.int32, device=dev)
        self.d_point_flags = torch.zeros((N, P), dtype=torch.uint8, device=dev)
        self._held_local = held
        self._n_frames_local = self.frames.n_f if n_frames is None else n_frames
        self.run_local_map(stream)

    def run_local_map(self, stream=None):
        """the call for the jobs `local_map` uploaded last, again (no allocation, no upload)"""
        orbgpu._check(_lib().orbgpu_track_local_map_batch_device(
            self.n_local, self.d_local_jobs.data_ptr(), self._n_frames_local, self.frames.d_table.data_ptr(),
            self.stride, self.point_stride, self.local_ws.data_ptr(), self.d_local_results.data_ptr(),
            self.d_local_rows.data_ptr(), self.d_point_flags.data_ptr(), orbgpu._stream_ptr(stream)),
            "orbgpu_track_local_map_batch_device")

    def local_results(self):
        return loop._struct_rows(self.d_local_results, TrackLocalResult, self.n_local)

    def local_rows(self):
        """(n, 3, stride) int32 by frame keypoint: mvpMapPoints after SearchLocalPoints, at the end; mvbOutlier"""
        return self.d_local_rows[:self.n_local].cpu().numpy()

    def point_flags(self):
        """(n, point_stride) uint8 of PT_SEEN / PT_IN_VIEW per table entry"""
        return self.d_point_flags[:self.n_local].cpu().numpy()


def update_last_frame(frames, stride=None, device="cuda", stream=None):
    """UpdateLastFrame's visual-odometry points for a list of frames, each a
    dict: depth (n,) f32 (mvDepth), kps (n,) orbgpu.KP_DTYPE (mvKeysUn), desc
    (n, 32) u8, K = (fx, fy, cx, cy, invfx, invfy), Rwc (3, 3), Ow (3,),
    th_depth, and the slot table flags (n,) int32, pos (n, 3) f32, mp_desc
    (n, 32) u8; optionally n (the count the job states, default len(depth)).
    Returns per frame a dict: status, n_created, n_pos, n_visited, created
    (n,) u8, flags, pos, mp_desc (the table after the call)."""
    import torch
    n = len(frames)
    S = int(stride) if stride is not None else max([len(f["depth"]) for f in frames] + [1])
    tab = (UpdateLastFrameJob * max(n, 1))()
    held = []
    for J, f in zip(tab, frames):
        t = {"depth": _up(f["depth"], np.float32, device), "kps": _up(f["kps"], orbgpu.KP_DTYPE, device),
             "desc": _up(f["desc"], np.uint8, device), "flags": _up(f["flags"], np.int32, device),
             "pos": _up(f["pos"], np.float32, device), "mp_desc": _up(f["mp_desc"], np.uint8, device)}
        held.append(t)
        J.n, J.th_depth = int(f.get("n", len(f["depth"]))), float(f["th_depth"])
        J.depth, J.kps_un, J.frame_desc = _ptr(t["depth"]), _ptr(t["kps"]), _ptr(t["desc"])
        J.fx, J.fy, J.cx, J.cy, J.invfx, J.invfy = (float(v) for v in f["K"])
        J.Rwc[:] = [float(v) for v in np.asarray(f["Rwc"], np.float32).reshape(9)]
        J.Ow[:] = [float(v) for v in np.asarray(f["Ow"], np.float32).reshape(3)]
        J.flags, J.pos, J.desc = _ptr(t["flags"]), _ptr(t["pos"]), _ptr(t["mp_desc"])
    d_jobs = bow.to_device_table(tab, device)
    d_res = torch.zeros(max(n, 1) * ctypes.sizeof(UpdateLastFrameResult), dtype=torch.uint8, device=device)
    d_created = torch.full((max(n, 1), S), 7, dtype=torch.uint8, device=device)
    orbgpu._check(_lib().orbgpu_update_last_frame_batch_device(n, d_jobs.data_ptr(), S, d_res.data_ptr(),
                                                               d_created.data_ptr(), orbgpu._stream_ptr(stream)),
                  "orbgpu_update_last_frame_batch_device")
    torch.cuda.synchronize()
    res = loop._struct_rows(d_res, UpdateLastFrameResult, n)
    created = d_created.cpu().numpy()
    out = []
    for k, (f, t) in enumerate(zip(frames, held)):
        m = len(f["depth"])
        out.append({"status": res[k].status, "n_created": res[k].n_created, "n_pos": res[k].n_pos,
                    "n_visited": res[k].n_visited, "created": created[k, :min(m, S)].copy(),
                    "flags": t["flags"].cpu().numpy().view(np.int32).copy(),
                    "pos": t["pos"].cpu().numpy().view(np.float32).reshape(-1, 3).copy(),
                    "mp_desc": t["mp_desc"].cpu().numpy().reshape(-1, 32).copy()})
    return out
