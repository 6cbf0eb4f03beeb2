"""Host-side mirror of Tracking::Relocalization's candidate loop over the C ABI
in include/orbgpu_reloc.h (csrc/reloc.hip).

* ``Frames`` -- the lost frames (mvKeysUn, descriptors, mvuRight, intrinsics,
  bounds, the scale pyramid) resident in HBM, plus their DBoW2 FeatureVectors
  (Frame::ComputeBoW).
* ``RelocBurst`` -- a batch of Relocalization() calls (src/Tracking.cpp:1747-1914),
  one query per lost frame: SearchByBoW(pKF, F) with ORBmatcher(0.75, true) for
  every candidate keyframe (:1786), the PnPsolver constructors of the candidates
  with >= 15 matches (:1787-1799), then the whole
  `while (nCandidates > 0 && !bMatch)` loop with its verification on the device
  (orbgpu_relocalize_batch_device).

The candidate keyframes are a ``loop.Keyframes`` with its ``loop.KeyframeSearch``.
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
import ransac

_BOUND = False

PENDING, MATCHED, NO_MATCH, CAPACITY = 0, 1, 2, 3
MAX_CANDIDATES = loop.MAX_CANDIDATES
MIN_MATCHES = 15
ROWS = 5
ROW_INLIERS, ROW_STAGE1, ROW_STAGE2, ROW_STAGE3, ROW_OUTLIER = range(ROWS)


class RelocFrame(ctypes.Structure):
    _fields_ = [("target", proj.Target), ("level_sigma2", ctypes.c_float * 16),
                ("inv_level_sigma2", ctypes.c_float * 16)]


class RelocCandidate(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_int), ("kf", ctypes.c_int)]


RelocQuery = loop.ComputeSim3Query


class RelocResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("matched", ctypes.c_int), ("round", ctypes.c_int), ("calls", ctypes.c_int),
                ("verifications", ctypes.c_int), ("hypotheses", ctypes.c_int), ("draws", ctypes.c_int),
                ("last_cand", ctypes.c_int), ("n_inliers", ctypes.c_int), ("refined", ctypes.c_int),
                ("nadditional", ctypes.c_int * 2), ("n_good", ctypes.c_int), ("pad", ctypes.c_int),
                ("pnp_Tcw", ctypes.c_float * 16), ("Tcw", ctypes.c_float * 16), ("opt", poseopt.PoseOptResult * 3),
                ("rng_after", ransac.RandState)]


class RelocCandidateState(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("min_inliers", ctypes.c_int), ("max_iterations", ctypes.c_int),
                ("iterations", ctypes.c_int), ("best_inliers", ctypes.c_int), ("discarded", ctypes.c_int)]


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        vp, i = ctypes.c_void_p, ctypes.c_int
        L.orbgpu_reloc_setup_workspace_bytes.argtypes = [i, i]
        L.orbgpu_reloc_setup_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_reloc_setup_batch_device.argtypes = [i, vp, vp, vp, vp, i, vp, vp, vp, vp]
        L.orbgpu_relocalize_workspace_bytes.argtypes = [i, i, i]
        L.orbgpu_relocalize_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_relocalize_batch_device.argtypes = [i, vp, i, vp, vp, vp, vp, vp, i, vp, i, i, vp, vp, vp, vp, vp]
        _BOUND = True
    return L


class Frames:
    """n_f lost frames of up to `stride` keypoints in HBM.  Host inputs (numpy):
    kps (n_f, stride) orbgpu.KP_DTYPE (mvKeysUn), desc (n_f, stride, 32) u8,
    u_right (n_f, stride) f32 or None (monocular), K (fx, fy, cx, cy), bf,
    bounds (min_x, max_x, min_y, max_y), scale_factors / level_sigma2 /
    inv_level_sigma2 (nlevels,) f32, log_scale_factor, counts (n_f,) (default
    all stride)."""

    def __init__(self, kps, desc, u_right, K, bf, bounds, scale_factors, level_sigma2, inv_level_sigma2,
                 log_scale_factor, counts=None, device="cuda"):
        import torch
        n_f, S = desc.shape[:2]
        self.n_f, self.stride, self.device = n_f, S, torch.device(device)
        self.counts_host = np.full(n_f, S, np.int32) if counts is None else np.asarray(counts, np.int32)
        kps = np.ascontiguousarray(kps, orbgpu.KP_DTYPE).reshape(n_f, S)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)  # noqa: E731
        self.kps = torch.from_numpy(kps.view(np.uint8).copy()).to(self.device)
        self.desc = up(desc, np.uint8)
        self.angle = up(kps["angle"], np.float32)
        self.ones = up(np.ones((n_f, S)), np.uint8)  # SearchByBoW(KF, F) asks nothing of the frame's MapPoints
        self.counts = up(self.counts_host, np.int32)
        self.u_right = None if u_right is None else up(u_right, np.float32)
        tab = (RelocFrame * n_f)()
        kpb = orbgpu.KP_DTYPE.itemsize
        for f in range(n_f):
            r, t = tab[f], tab[f].target
            t.n = int(self.counts_host[f])
            t.kps = self.kps.data_ptr() + kpb * S * f
            t.desc = self.desc.data_ptr() + 32 * S * f
            t.u_right = None if self.u_right is None else self.u_right.data_ptr() + 4 * S * f
            t.min_x, t.max_x, t.min_y, t.max_y = (float(v) for v in bounds)
            t.fx, t.fy, t.cx, t.cy = (float(v) for v in K)
            t.bf = float(bf)
            t.n_levels = len(scale_factors)
            t.log_scale_factor = float(log_scale_factor)
            t.scale_factors[:len(scale_factors)] = [float(v) for v in scale_factors]
            r.level_sigma2[:len(level_sigma2)] = [float(v) for v in level_sigma2]
            r.inv_level_sigma2[:len(inv_level_sigma2)] = [float(v) for v in inv_level_sigma2]
        self.d_table = bow.to_device_table(tab, self.device)
        self.tf = None

    def compute_bow(self, voc: bow.Vocabulary, levelsup=4, stream=None):
        """Frame::ComputeBoW for every frame (mFeatVec, levelsup 4)."""
        self.tf = bow.BatchTransform(self.n_f, self.stride, self.device)
        bow.transform_batch(voc, self.desc, self.counts, self.tf, levelsup, stream)
        self.frames = bow.frame_table(self.tf, self.desc, self.angle, self.ones, self.counts_host)
        return self.tf


class RelocBurst:
    """Relocalization() for `queries` = list of (frame, [candidate kfs], rng
    state or seed): all SearchByBoW pairs in one batch, then the PnPsolver
    set-up and the loop of every query on the GPU."""

    def __init__(self, frames: Frames, kfs: loop.Keyframes, search: loop.KeyframeSearch, queries, nnratio=0.75,
                 check_ori=True, match=None, nmatches=None):
        """match (pairs, stride) / nmatches (pairs,): SearchByBoW's results from
        elsewhere, uploaded instead of computed (no vocabulary needed;
        search_by_bow is then not available)."""
        import torch
        if frames.stride != kfs.stride:
            raise ValueError("frames and keyframes must share the stride")
        if match is None and (frames.tf is None or kfs.tf is None):
            raise ValueError("Frames.compute_bow() and Keyframes.compute_bow() first")
        self.frames, self.kfs, self.search = frames, kfs, search
        self.nnratio, self.check_ori = nnratio, check_ori
        dev, S = kfs.device, kfs.stride
        pairs, qtab = [], (RelocQuery * max(len(queries), 1))()
        for qi, (f, cands, rng) in enumerate(queries):
            if len(cands) > MAX_CANDIDATES:
                raise ValueError(f"at most {MAX_CANDIDATES} candidates per query")
            qtab[qi].first_cand, qtab[qi].n_cand = len(pairs), len(cands)
            if isinstance(rng, ransac.RandState):
                qtab[qi].rng = rng
            else:
                orbgpu.lib().orbgpu_srand_r(ctypes.byref(qtab[qi].rng), int(rng) & 0xFFFFFFFF)
            pairs.extend((f, c) for c in cands)
        self.n_queries, self.n_pairs = len(queries), len(pairs)
        self.pairs = np.array(pairs, np.int32).reshape(-1, 2)
        P, Q = max(self.n_pairs, 1), max(self.n_queries, 1)
        ctab = (RelocCandidate * P)()
        fa, fb = (bow.BowFrame * P)(), (bow.BowFrame * P)()
        for p, (f, k) in enumerate(pairs):
            ctab[p].frame, ctab[p].kf = f, k
            if match is None:
                fa[p], fb[p] = kfs.frames[k], frames.frames[f]  # A = KF, B = F
        self.d_fa, self.d_fb = bow.to_device_table(fa, dev), bow.to_device_table(fb, dev)
        self.d_cands = bow.to_device_table(ctab, dev)
        self.d_queries = bow.to_device_table(qtab, dev)
        self.uploaded = match is not None
        self.match = torch.zeros((P, S), dtype=torch.int32, device=dev)
        self.nmatches = torch.zeros(P, dtype=torch.int32, device=dev)
        if self.uploaded:
            self.match.copy_(torch.from_numpy(np.ascontiguousarray(match, np.int32).reshape(P, S)))
            self.nmatches.copy_(torch.from_numpy(np.ascontiguousarray(nmatches, np.int32).reshape(P)))
        L = _lib()
        self.n_corr = torch.zeros(P, dtype=torch.int32, device=dev)
        self.workspace = torch.zeros(L.orbgpu_reloc_setup_workspace_bytes(P, S), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(L.orbgpu_relocalize_workspace_bytes(Q, P, S), dtype=torch.uint8, device=dev)
        self.results = torch.zeros(Q * ctypes.sizeof(RelocResult), dtype=torch.uint8, device=dev)
        self.cand_states = torch.zeros(P * ctypes.sizeof(RelocCandidateState), dtype=torch.uint8, device=dev)
        self.rows = torch.zeros((Q, ROWS, S), dtype=torch.int32, device=dev)
        self.started = False

    @classmethod
    def from_tables(cls, frames: Frames, kfs: loop.Keyframes, search: loop.KeyframeSearch, tables, nnratio=0.75,
                    check_ori=True):
        """A burst over prepared device tables (kfdb.RelocTables, filled on the
        device by kfdb.KeyFrameDatabase.emit_reloc): query q owns entries
        [q * cand_stride, (q + 1) * cand_stride) and its candidates are known
        on the device only, so ``pairs`` is not available.  Nothing is read
        back or uploaded here."""
        import torch
        if frames.stride != kfs.stride:
            raise ValueError("frames and keyframes must share the stride")
        self = cls.__new__(cls)
        self.frames, self.kfs, self.search = frames, kfs, search
        self.nnratio, self.check_ori = nnratio, check_ori
        dev, S = kfs.device, kfs.stride
        self.n_queries, self.n_pairs = tables.n_queries, tables.n_queries * tables.cand_stride
        self.pairs, self.tables = None, tables
        P, Q = max(self.n_pairs, 1), max(self.n_queries, 1)
        self.d_fa, self.d_fb, self.d_cands, self.d_queries = tables.d_fa, tables.d_fb, tables.d_cands, tables.d_queries
        self.uploaded = False
        self.match = torch.zeros((P, S), dtype=torch.int32, device=dev)
        self.nmatches = torch.zeros(P, dtype=torch.int32, device=dev)
        L = _lib()
        self.n_corr = torch.zeros(P, dtype=torch.int32, device=dev)
        self.workspace = torch.zeros(L.orbgpu_reloc_setup_workspace_bytes(P, S), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(L.orbgpu_relocalize_workspace_bytes(Q, P, S), dtype=torch.uint8, device=dev)
        self.results = torch.zeros(Q * ctypes.sizeof(RelocResult), dtype=torch.uint8, device=dev)
        self.cand_states = torch.zeros(P * ctypes.sizeof(RelocCandidateState), dtype=torch.uint8, device=dev)
        self.rows = torch.zeros((Q, ROWS, S), dtype=torch.int32, device=dev)
        self.started = False
        return self

    def search_by_bow(self, stream=None):
        """SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]) for every pair."""
        if self.uploaded:
            raise ValueError("the SearchByBoW rows were uploaded")
        bow.search_by_bow_batch(bow.KF_F, self.d_fa, self.d_fb, self.n_pairs, self.nnratio, self.check_ori,
                                self.kfs.stride, self.match, self.nmatches, stream)

    def setup(self, stream=None):
        """PnPsolver(mCurrentFrame, matches) + SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) per candidate."""
        orbgpu._check(_lib().orbgpu_reloc_setup_batch_device(
            self.n_pairs, self.d_cands.data_ptr(), self.frames.d_table.data_ptr(), self.kfs.d_table.data_ptr(),
            self.match.data_ptr(), self.kfs.stride, self.nmatches.data_ptr(), self.workspace.data_ptr(),
            self.n_corr.data_ptr(), orbgpu._stream_ptr(stream)), "orbgpu_reloc_setup_batch_device")

    def relocalize(self, n_passes=1, resume=False, stream=None):
        """n_passes passes of the loop (orbgpu_relocalize_batch_device)."""
        if resume and not self.started:
            raise ValueError("nothing to resume")
        orbgpu._check(_lib().orbgpu_relocalize_batch_device(
            self.n_queries, self.d_queries.data_ptr(), self.n_pairs, self.d_cands.data_ptr(),
            self.frames.d_table.data_ptr(), self.kfs.d_table.data_ptr(), self.search.d_table.data_ptr(),
            self.match.data_ptr(), self.kfs.stride, self.workspace.data_ptr(), int(n_passes),
            int(bool(resume)), self.state.data_ptr(), self.results.data_ptr(), self.cand_states.data_ptr(),
            self.rows.data_ptr(), orbgpu._stream_ptr(stream)), "orbgpu_relocalize_batch_device")
        self.started = True

    def step(self, n_passes=1, stream=None, max_calls=1 << 20):
        """The reference's whole loop for every query: the PnPsolver set-up
        (after SearchByBoW unless the rows were uploaded), then calls of
        n_passes passes each until no query is PENDING.  Returns the number
        of calls."""
        if not self.uploaded:
            self.search_by_bow(stream)
        self.setup(stream)
        calls = 0
        while calls < max_calls:
            self.relocalize(n_passes, resume=calls > 0, stream=stream)
            calls += 1
            if not any(r.status == PENDING for r in self.query_results()):
                break
        return calls

    # ---- results (host) ---------------------------------------------------
    def query_results(self):
        return loop._struct_rows(self.results, RelocResult, self.n_queries)

    def candidate_states(self):
        return loop._struct_rows(self.cand_states, RelocCandidateState, self.n_pairs)

    def query_rows(self):
        """(n_queries, ROWS, stride) int32 of each query's last verification, by
        frame keypoint: vbInliers, mvpMapPoints after the first optimisation and
        its cull, after the second optimisation, at the end; mvbOutlier."""
        return self.rows[:self.n_queries].cpu().numpy()

    def n_correspondences(self):
        return self.n_corr[:self.n_pairs].cpu().numpy()
