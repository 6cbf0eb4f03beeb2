"""Host-side mirror of the keyframe database on the device over the C ABI in
include/orbgpu_kfdb.h (csrc/kfdb.hip).

* ``KeyFrameDatabase`` -- every keyframe's BowVector, the add()/erase() state,
  the ten best covisibles and mRelocScore, resident in HBM.  ``add`` and
  ``erase`` are host-side and re-upload their arrays.
* ``KeyFrameDatabase.detect`` -- DetectRelocalizationCandidates /
  DetectLoopCandidates (src/KeyFrameDatabase.cpp:96-361) for a batch of queries
  (orbgpu_kfdb_detect_batch_device), asynchronous on the stream.
* ``KeyFrameDatabase.emit_reloc`` -- the relocalisation candidates as the device
  tables ``reloc.RelocBurst.from_tables`` takes, so ComputeBoW -> detect ->
  SearchByBoW -> PnPsolver set-up -> the candidate loop runs on one stream.

Everything runs on the GPU; there is no host fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

import bow
import loop
import orbgpu
import ransac
import reloc

_BOUND = False

RELOC, LOOP = 0, 1
OK, CAPACITY, BAD_JOB = 0, 1, 2
MAX_KEYFRAMES = 8192
MAX_WORDS = 4096
COVIS = 10

_vp = ctypes.c_void_p


class KfdbStruct(ctypes.Structure):
    _fields_ = [("n_kf", ctypes.c_int), ("scoring", ctypes.c_int), ("n_bow_total", ctypes.c_int),
                ("pad", ctypes.c_int), ("in_db", _vp), ("add_rank", _vp), ("kf_bad", _vp), ("bow_offset", _vp),
                ("n_bow", _vp), ("bow_words", _vp), ("bow_values", _vp), ("covis", _vp), ("reloc_score", _vp)]


class KfdbQuery(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("n_words", ctypes.c_int), ("n_connected", ctypes.c_int),
                ("n_covisible", ctypes.c_int), ("min_score", ctypes.c_float), ("pad", ctypes.c_int), ("words", _vp),
                ("values", _vp), ("d_n_words", _vp), ("connected", _vp), ("covisible", _vp)]


class KfdbResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_sharing", ctypes.c_int), ("max_common", ctypes.c_int),
                ("min_common", ctypes.c_int), ("n_filtered", ctypes.c_int), ("n_scored", ctypes.c_int),
                ("n_candidates", ctypes.c_int), ("min_score", ctypes.c_float), ("best_acc_score", ctypes.c_float),
                ("pad", ctypes.c_int)]


def _lib():
    global _BOUND
    L = orbgpu.lib()
    if not _BOUND:
        i = ctypes.c_int
        L.orbgpu_kfdb_detect_workspace_bytes.argtypes = [i, i]
        L.orbgpu_kfdb_detect_workspace_bytes.restype = ctypes.c_size_t
        L.orbgpu_kfdb_detect_batch_device.argtypes = [i, _vp, _vp, i, _vp, _vp, _vp, _vp, _vp, _vp]
        L.orbgpu_kfdb_emit_reloc_batch_device.argtypes = [i, _vp, _vp, _vp, i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        _BOUND = True
    return L


def _up(a, dtype, device):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        a = np.zeros(1, dtype)
    return torch.from_numpy(a.copy()).to(device)


def set_fv_n(d_table, tf: bow.BatchTransform):
    """fv_n of every record of a frame_table_device table from tf.fv_n, on the
    device (torch's current stream)"""
    import torch
    ints = d_table.view(torch.int32).view(max(tf.B, 1), ctypes.sizeof(bow.BowFrame) // 4)
    ints[:tf.B, bow.BowFrame.fv_n.offset // 4] = tf.fv_n


def frame_table_device(tf: bow.BatchTransform, desc, angle, valid, counts_host, fill=True):
    """bow.frame_table as a device table without reading the transform's counts
    back: the records are built from the addresses and the host's feature
    counts; fv_n is copied from tf.fv_n on the device, here (fill, after
    transform_batch) or later by set_fv_n (the table built before the chain)."""
    S = tf.stride
    tab = (bow.BowFrame * max(tf.B, 1))()
    for b in range(tf.B):
        tab[b] = bow.BowFrame(int(counts_host[b]), 0, tf.fv_nodes.data_ptr() + 4 * S * b,
                              tf.fv_offsets.data_ptr() + 4 * (S + 1) * b, tf.fv_features.data_ptr() + 4 * S * b,
                              desc.data_ptr() + 32 * S * b, angle.data_ptr() + 4 * S * b, valid.data_ptr() + S * b)
    d = bow.to_device_table(tab, desc.device)
    if fill:
        set_fv_n(d, tf)
    return d


class Queries:
    """A batch of queries on the device.  Each is a dict:
    kind (RELOC / LOOP); bow, a dict word -> value, or device=(words_ptr,
    values_ptr, n_words_ptr), a BowVector already in HBM whose count is read on
    the device (bow.transform_batch's rows); LOOP: connected (keyframe indices),
    covisible (indices, or None to take min_score as given), min_score."""

    def __init__(self, queries, device):
        self.n = len(queries)
        self.keep = []
        tab = (KfdbQuery * max(self.n, 1))()
        for q, spec in zip(tab, queries):
            q.kind = int(spec["kind"])
            if "device" in spec:
                q.words, q.values, q.d_n_words = spec["device"]
            else:
                ws = sorted(spec["bow"])
                w, v = _up(ws, np.int32, device), _up([spec["bow"][x] for x in ws], np.float64, device)
                self.keep += [w, v]
                q.n_words, q.words, q.values = len(ws), w.data_ptr(), v.data_ptr()
            conn = list(spec.get("connected", ()))
            c = _up(conn, np.int32, device)
            self.keep.append(c)
            q.n_connected, q.connected = len(conn), c.data_ptr()
            cov = spec.get("covisible")
            q.n_covisible = -1
            if cov is not None:
                c = _up(list(cov), np.int32, device)
                self.keep.append(c)
                q.n_covisible, q.covisible = len(cov), c.data_ptr()
            q.min_score = float(spec.get("min_score", 0.0))
            for name, value in spec.get("raw", {}).items():  # a field as given (tests of the checks)
                setattr(q, name, value)
        self.tab = tab
        self.d_table = bow.to_device_table(tab, device)


class Detection:
    """What detect() left on the device."""

    def __init__(self, n, n_kf, cand_stride, rows, device):
        import torch
        N, K = max(n, 1), max(n_kf, 1)
        self.n, self.n_kf, self.cand_stride = n, n_kf, cand_stride
        self.results = torch.zeros(N * ctypes.sizeof(KfdbResult), dtype=torch.uint8, device=device)
        self.candidates = torch.full((N, cand_stride), -1, dtype=torch.int32, device=device)
        self.words = torch.zeros((N, K), dtype=torch.int32, device=device) if rows else None
        self.scores = torch.zeros((N, K), dtype=torch.float32, device=device) if rows else None

    def query_results(self):
        return loop._struct_rows(self.results, KfdbResult, self.n)

    def candidate_lists(self):
        """per query the candidates written (all of them unless CAPACITY)"""
        c = self.candidates.cpu().numpy()
        return [[int(x) for x in c[q, :min(r.n_candidates, self.cand_stride)]]
                for q, r in enumerate(self.query_results())]


class RelocTables:
    """The device tables of one relocalisation burst, n_queries * cand_stride
    entries: allocated (with each query's random state) before the chain,
    filled by KeyFrameDatabase.emit_reloc."""

    def __init__(self, n_queries, cand_stride, rngs, device):
        if not 1 <= cand_stride <= reloc.MAX_CANDIDATES:
            raise ValueError(f"cand_stride must be 1..{reloc.MAX_CANDIDATES}")
        import torch
        self.n_queries, self.cand_stride = n_queries, cand_stride
        P = max(n_queries * cand_stride, 1)
        qtab = (reloc.RelocQuery * max(n_queries, 1))()
        for q, rng in zip(qtab, rngs):
            if isinstance(rng, ransac.RandState):
                q.rng = rng
            else:
                orbgpu.lib().orbgpu_srand_r(ctypes.byref(q.rng), int(rng) & 0xFFFFFFFF)
        self.d_queries = bow.to_device_table(qtab, device)
        zeros = lambda struct: torch.zeros(P * ctypes.sizeof(struct), dtype=torch.uint8, device=device)  # noqa: E731
        self.d_cands, self.d_fa, self.d_fb = zeros(reloc.RelocCandidate), zeros(bow.BowFrame), zeros(bow.BowFrame)

    def candidates(self):
        return loop._struct_rows(self.d_cands, reloc.RelocCandidate, self.n_queries * self.cand_stride)

    def queries(self):
        return loop._struct_rows(self.d_queries, reloc.RelocQuery, self.n_queries)


class KeyFrameDatabase:
    """bows: per keyframe (map-mirror index) a dict word -> value, mBowVec;
    covis (n_kf, 10) int32, -1 padded; kf_bad (n_kf,) or None; reloc_score
    (n_kf,) float32, what mRelocScore holds (default zeros).  No keyframe is in
    the database until add()ed."""

    def __init__(self, bows, covis, scoring, kf_bad=None, reloc_score=None, device="cuda"):
        import torch
        self.device = torch.device(device)
        self.n_kf, self.scoring = len(bows), int(scoring)
        if self.n_kf > MAX_KEYFRAMES:
            raise ValueError(f"at most {MAX_KEYFRAMES} keyframes")
        off, nb, words, vals = [], [], [], []
        for b in bows:
            ws = sorted(b)
            off.append(len(words))
            nb.append(len(ws))
            words += ws
            vals += [b[w] for w in ws]
        self.n_bow_total = len(words)
        dev = self.device
        self.bow_offset, self.n_bow = _up(off, np.int32, dev), _up(nb, np.int32, dev)
        self.bow_words, self.bow_values = _up(words, np.int32, dev), _up(vals, np.float64, dev)
        self.covis = _up(np.asarray(covis, np.int32).reshape(self.n_kf, COVIS), np.int32, dev)
        self.kf_bad = _up(np.zeros(self.n_kf) if kf_bad is None else kf_bad, np.uint8, dev)
        self.reloc_score = _up(np.zeros(self.n_kf) if reloc_score is None else reloc_score, np.float32, dev)
        self.in_db_host = np.zeros(max(self.n_kf, 1), np.uint8)
        self.add_rank_host = np.zeros(max(self.n_kf, 1), np.int32)
        self.n_added = 0
        self._upload_state()
        self.workspace = None

    @classmethod
    def from_transform(cls, tf: bow.BatchTransform, covis, scoring, kf_bad=None, reloc_score=None):
        """The keyframes' BowVectors where bow.transform_batch leaves them: row
        k of `tf` is keyframe k, its count read on the device (a row the
        transform rejected makes the queries that read it BAD_JOB).  Nothing
        is copied, so the transform may still be in flight on the stream."""
        import torch
        self = cls([], np.zeros((0, COVIS)), scoring, device=tf.bow_n.device)
        dev, S = self.device, tf.stride
        self.n_kf, self.n_bow_total, self.tf = tf.B, tf.B * S, tf
        self.bow_offset = torch.arange(tf.B, dtype=torch.int32, device=dev) * S
        self.n_bow, self.bow_words, self.bow_values = tf.bow_n, tf.bow_words, tf.bow_values
        self.covis = _up(np.asarray(covis, np.int32).reshape(self.n_kf, COVIS), np.int32, dev)
        self.kf_bad = _up(np.zeros(self.n_kf) if kf_bad is None else kf_bad, np.uint8, dev)
        self.reloc_score = _up(np.zeros(self.n_kf) if reloc_score is None else reloc_score, np.float32, dev)
        self.in_db_host = np.zeros(max(self.n_kf, 1), np.uint8)
        self.add_rank_host = np.zeros(max(self.n_kf, 1), np.int32)
        self._upload_state()
        return self

    def _upload_state(self):
        self.in_db = _up(self.in_db_host, np.uint8, self.device)
        self.add_rank = _up(self.add_rank_host, np.int32, self.device)

    def add(self, *kfs):
        """KeyFrameDatabase::add, in call order"""
        for k in kfs:
            self.in_db_host[k] = 1
            self.add_rank_host[k] = self.n_added
            self.n_added += 1
        self._upload_state()

    def erase(self, *kfs):
        for k in kfs:
            self.in_db_host[k] = 0
        self._upload_state()

    def set_bad(self, kf_bad):
        self.kf_bad = _up(kf_bad, np.uint8, self.device)

    def struct(self) -> KfdbStruct:
        return KfdbStruct(self.n_kf, self.scoring, self.n_bow_total, 0, self.in_db.data_ptr(), self.add_rank.data_ptr(),
                          self.kf_bad.data_ptr(), self.bow_offset.data_ptr(), self.n_bow.data_ptr(),
                          self.bow_words.data_ptr(), self.bow_values.data_ptr(), self.covis.data_ptr(),
                          self.reloc_score.data_ptr())

    def queries(self, queries) -> Queries:
        return Queries(queries, self.device)

    def reserve(self, n_queries):
        """the opaque block for batches of up to n_queries, allocated ahead of a chain"""
        import torch
        need = _lib().orbgpu_kfdb_detect_workspace_bytes(n_queries, self.n_kf)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)

    def detect(self, queries, cand_stride, rows=False, stream=None, struct=None, out=None) -> Detection:
        """queries: a Queries or the list it is built from.  rows: also the
        per-(query, keyframe) common-word counts and scores.  out: a Detection
        allocated earlier (with reserve() and a prepared Queries the call then
        allocates and uploads nothing).  struct: the database struct to pass
        instead of the object's own."""
        if not isinstance(queries, Queries):
            queries = Queries(queries, self.device)
        L = _lib()
        det = Detection(queries.n, self.n_kf, cand_stride, rows, self.device) if out is None else out
        rows = det.words is not None
        self.reserve(queries.n)
        det.queries = queries
        D = self.struct() if struct is None else struct
        orbgpu._check(L.orbgpu_kfdb_detect_batch_device(
            queries.n, queries.d_table.data_ptr(), ctypes.addressof(D), cand_stride, self.workspace.data_ptr(),
            det.results.data_ptr(), det.candidates.data_ptr(), det.words.data_ptr() if rows else None,
            det.scores.data_ptr() if rows else None, orbgpu._stream_ptr(stream)), "orbgpu_kfdb_detect_batch_device")
        return det

    def emit_reloc(self, det: Detection, d_frame_of_query, d_kf_bow, d_frame_bow, tables: RelocTables, stream=None):
        """Fill `tables` from a detection: d_frame_of_query (n,) int32 on the
        device, d_kf_bow / d_frame_bow device tables of orbgpu_bow_frame by
        keyframe / by frame.  Returns `tables`."""
        if tables.n_queries != det.n or tables.cand_stride != det.cand_stride:
            raise ValueError("the tables were allocated for another batch")
        orbgpu._check(_lib().orbgpu_kfdb_emit_reloc_batch_device(
            det.n, d_frame_of_query.data_ptr(), det.results.data_ptr(), det.candidates.data_ptr(), det.cand_stride,
            self.kf_bad.data_ptr(), d_kf_bow.data_ptr(), d_frame_bow.data_ptr(), tables.d_cands.data_ptr(),
            tables.d_queries.data_ptr(), tables.d_fa.data_ptr(), tables.d_fb.data_ptr(), orbgpu._stream_ptr(stream)),
            "orbgpu_kfdb_emit_reloc_batch_device")
        return tables
