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
  either the caller's (``local_map`` takes a host-built table and can read the
  pose ``initial`` left in place) or ``update_local_map`` (:1571-1745,
  include/orbgpu_localmap.h, csrc/localmap.hip), which reads ``initial``'s rows
  in place and a ``MapMirror`` and fills the buffers ``prepare_local_map``
  allocated: ``run_initial; run_update_local_map; run_local_map`` is then three
  launches on one stream and no upload.
* ``MapMirror`` -- the map's keyframes and points as plain arrays in HBM.
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


LM_OK, LM_KEPT, LM_CAPACITY, LM_BAD_JOB = range(4)  # ORBGPU_LOCALMAP_*


class MapMirrorStruct(ctypes.Structure):
    _fields_ = [("n_kf", ctypes.c_int), ("n_pt", ctypes.c_int), ("n_slots_total", ctypes.c_int),
                ("n_children_total", ctypes.c_int), ("n_obs_total", ctypes.c_int), ("pad", ctypes.c_int),
                ("kf_bad", vp), ("slot_offset", vp), ("n_slots", vp), ("slots", vp), ("covis", vp),
                ("child_offset", vp), ("n_children", vp), ("children", vp), ("parent", vp), ("kf_by_rank", vp),
                ("pt_flags", vp), ("obs_offset", vp), ("n_obs", vp), ("obs", vp), ("pos", vp), ("normal", vp),
                ("desc", vp), ("min_dist", vp), ("max_dist", vp)]


class UpdateLocalMapJob(ctypes.Structure):
    _fields_ = [("n_kp", ctypes.c_int), ("src_n", ctypes.c_int), ("n_prev_kfs", ctypes.c_int), ("pad", ctypes.c_int),
                ("rows", vp), ("src_pt_id", vp), ("src_pos", vp), ("src_desc", vp), ("prev_kfs", vp),
                ("out_flags", vp), ("out_pos", vp), ("out_normal", vp), ("out_desc", vp), ("out_min_dist", vp),
                ("out_max_dist", vp), ("frame_mp", vp), ("local_job", vp)]


class UpdateLocalMapResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_k1", ctypes.c_int), ("n_local_kfs", ctypes.c_int),
                ("ref_kf", ctypes.c_int), ("n_nulled", ctypes.c_int), ("n_local", ctypes.c_int),
                ("n_extra", ctypes.c_int), ("pad", ctypes.c_int)]


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
        L.orbgpu_update_local_map_workspace_bytes.argtypes = [i, i, i, i, i, i]
        L.orbgpu_update_local_map_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_update_local_map_batch_device.argtypes = [i, vp, ctypes.POINTER(MapMirrorStruct), i, i, i, vp, vp, vp,
                                                           vp, vp]
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


def _ragged(lists):
    """per-row offsets, counts and the concatenation of a list of int lists"""
    cnt = np.array([len(x) for x in lists], np.int32)
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in lists] + [np.zeros(0, np.int32)])
    return off, cnt, flat.astype(np.int32)


class MapMirror:
    """The map as Tracking::UpdateLocalMap reads it, uploaded from numpy (include/orbgpu_localmap.h): kf_bad
    (n_kf,), slots (per keyframe an int array of point ids, -1 = NULL), covis (n_kf, 10) -1 padded, children
    (per keyframe a list, in the order that stands for the std::set's), parent (n_kf,), kf_by_rank (None or a
    permutation: the order that stands for the std::map's); pt_flags (n_pt,) of proj.VALID / proj.HAS_OBS, obs
    (per point a list of keyframes), pos, normal (n_pt, 3), desc (n_pt, 32), min_dist, max_dist (n_pt,).  The
    caller keeps it current; many jobs and calls share one."""

    def __init__(self, kf_bad, slots, covis, children, parent, pt_flags, obs, pos, normal, desc, min_dist, max_dist,
                 kf_by_rank=None, device="cuda"):
        so, sn, sf = _ragged(slots)
        co, cn, cf = _ragged(children)
        oo, on, of = _ragged(obs)
        host = {"kf_bad": (kf_bad, np.uint8), "slot_offset": (so, np.int32), "n_slots": (sn, np.int32),
                "slots": (sf, np.int32), "covis": (covis, np.int32), "child_offset": (co, np.int32),
                "n_children": (cn, np.int32), "children": (cf, np.int32), "parent": (parent, np.int32),
                "pt_flags": (pt_flags, np.int32), "obs_offset": (oo, np.int32), "n_obs": (on, np.int32),
                "obs": (of, np.int32), "pos": (pos, np.float32), "normal": (normal, np.float32),
                "desc": (desc, np.uint8), "min_dist": (min_dist, np.float32), "max_dist": (max_dist, np.float32)}
        if kf_by_rank is not None:
            host["kf_by_rank"] = (kf_by_rank, np.int32)
        self.t = {name: _up(a, dt, device) for name, (a, dt) in host.items()}
        self.n_kf, self.n_pt = len(kf_bad), len(pt_flags)
        c = self.c = MapMirrorStruct()
        c.n_kf, c.n_pt = self.n_kf, self.n_pt
        c.n_slots_total, c.n_children_total, c.n_obs_total = len(sf), len(cf), len(of)
        for name, t in self.t.items():
            setattr(c, name, _ptr(t))


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


    # ---- 1b. UpdateLocalMap: call 2's table, frame_mp and job made on the device --------
    TABLE = (("flags", np.int32, ()), ("pos", np.float32, (3,)), ("normal", np.float32, (3,)), ("desc", np.uint8, (32,)),
             ("min_dist", np.float32, ()), ("max_dist", np.float32, ()))

    def prepare_local_map(self, jobs, point_stride, n_frames=None):
        """Allocates, once, everything call 2 reads and writes for len(jobs) frames: per frame a table of
        point_stride entries and a frame_mp row that update_local_map fills, the jobs (dicts with frame, Tcw --
        16 or 12 floats or a device address such as initial_pose_ptr(k) -- th and optionally stereo,
        only_tracking, recently_relocalised; n_local, points and frame_mp are the device's to write), the
        workspace, the results, the rows and the point flags.  Nothing is launched."""
        import torch
        n, S, dev, P = len(jobs), self.stride, self.device, int(point_stride)
        N = max(n, 1)
        tt = {"flags": torch.int32, "desc": torch.uint8}
        self.d_table = {name: torch.zeros((N, P) + shape, dtype=tt.get(name, torch.float32), device=dev)
                        for name, _, shape in self.TABLE}
        self.d_frame_mp = torch.zeros((N, S), dtype=torch.int32, device=dev)
        tab = (TrackLocalJob * N)()
        held = []
        for J, j in zip(tab, jobs):
            J.frame = int(j["frame"])
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
        L = _lib()
        self.n_local, self.point_stride = n, P
        self.d_local_jobs = bow.to_device_table(tab, dev)
        self.local_ws = torch.zeros(L.orbgpu_track_local_workspace_bytes(N, S, P), dtype=torch.uint8, device=dev)
        self.d_local_results = torch.zeros(N * ctypes.sizeof(TrackLocalResult), dtype=torch.uint8, device=dev)
        self.d_local_rows = torch.zeros((N, LOCAL_ROWS, S), dtype=torch.int32, device=dev)
        self.d_point_flags = torch.zeros((N, P), dtype=torch.uint8, device=dev)
        self._held_local = held
        self._n_frames_local = self.frames.n_f if n_frames is None else n_frames

    def update_local_map(self, jobs, mirror, stream=None, kf_stride=128, launch=True):
        """Tracking::UpdateLocalMap for the frames of prepare_local_map, one job each: dicts with n_kp,
        src_pt_id ((src_n,) int32: per entry of call 1's table the mirror's point id or -1), table (call 1's
        PointTable, read for the -1 entries' pos and desc; or None), prev_kfs (mvpLocalKeyFrames before the
        call) and optionally rows ((2, stride) int32, uploaded; default: job k reads initial's rows of job k in
        place).  Fills the tables, frame_mp and jobs that run_local_map then reads."""
        import torch
        n, S, dev, P, KS = len(jobs), self.stride, self.device, self.point_stride, int(kf_stride)
        assert n == self.n_local, "prepare_local_map() first, for as many frames"
        N = max(n, 1)
        tab = (UpdateLocalMapJob * N)()
        held = [mirror]
        sz = ctypes.sizeof(TrackLocalJob)
        for k, (J, j) in enumerate(zip(tab, jobs)):
            src = _up(j["src_pt_id"], np.int32, dev)
            prev = _up(j.get("prev_kfs", []), np.int32, dev)
            J.n_kp, J.src_n, J.n_prev_kfs = int(j["n_kp"]), int(j.get("src_n", src.numel() // 4)), prev.numel() // 4
            rows = j.get("rows")
            if rows is not None:
                r = np.full((2, S), -1, np.int32)
                rows = np.asarray(rows, np.int32)
                r[:, :min(rows.shape[1], S)] = rows[:, :S]
                rows = _up(r, np.int32, dev)
                J.rows = rows.data_ptr()
            else:
                J.rows = self.d_initial_rows.data_ptr() + k * INITIAL_ROWS * S * 4
            J.src_pt_id, J.prev_kfs = _ptr(src), _ptr(prev)
            t = j.get("table")
            if t is not None:
                J.src_pos, J.src_desc = _ptr(t.t.get("pos")), _ptr(t.t.get("desc"))
            for name, _, _ in self.TABLE:
                d = self.d_table[name]
                setattr(J, "out_" + name, d.data_ptr() + k * d.stride(0) * d.element_size())
            J.frame_mp = self.d_frame_mp.data_ptr() + k * S * 4
            J.local_job = self.d_local_jobs.data_ptr() + k * sz
            held += [src, prev, rows, t]
        L = _lib()
        self.mirror, self.kf_stride = mirror, KS
        self.d_lm_jobs = bow.to_device_table(tab, dev)
        self.lm_ws = torch.empty(L.orbgpu_update_local_map_workspace_bytes(N, S, P, KS, mirror.n_kf, mirror.n_pt),
                                 dtype=torch.uint8, device=dev)
        self.d_lm_results = torch.zeros(N * ctypes.sizeof(UpdateLocalMapResult), dtype=torch.uint8, device=dev)
        self.d_local_kfs = torch.zeros((N, KS), dtype=torch.int32, device=dev)
        self.d_local_points = torch.zeros((N, P), dtype=torch.int32, device=dev)
        self._held_lm = held
        if launch:
            self.run_update_local_map(stream)

    def run_update_local_map(self, stream=None):
        """the call for the jobs `update_local_map` uploaded last, again (no allocation, no upload)"""
        orbgpu._check(_lib().orbgpu_update_local_map_batch_device(
            self.n_local, self.d_lm_jobs.data_ptr(), ctypes.byref(self.mirror.c), self.stride, self.point_stride,
            self.kf_stride, self.lm_ws.data_ptr(), self.d_lm_results.data_ptr(), self.d_local_kfs.data_ptr(),
            self.d_local_points.data_ptr(), orbgpu._stream_ptr(stream)), "orbgpu_update_local_map_batch_device")

    def update_results(self):
        return loop._struct_rows(self.d_lm_results, UpdateLocalMapResult, self.n_local)

    def local_kfs(self):
        """(n, kf_stride) int32: mvpLocalKeyFrames; the first n_local_kfs of a row are written"""
        return self.d_local_kfs[:self.n_local].cpu().numpy()

    def local_points(self):
        """(n, point_stride) int32: the mirror ids of mvpLocalMapPoints; the first n_local of a row are written"""
        return self.d_local_points[:self.n_local].cpu().numpy()

    def prepared_tables(self):
        """call 2's tables as the device filled them: name -> (n, point_stride, ..) numpy"""
        return {name: t[:self.n_local].cpu().numpy() for name, t in self.d_table.items()}

    def prepared_frame_mp(self):
        return self.d_frame_mp[:self.n_local].cpu().numpy()

    def prepared_jobs(self):
        """call 2's jobs as they stand on the device"""
        return loop._struct_rows(self.d_local_jobs, TrackLocalJob, self.n_local)


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
