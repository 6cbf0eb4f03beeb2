"""KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling on the covisibility table in HBM
(include/orbgpu_covis.h, csrc/covis.hip, covis.py), against the sequential restatement
tests/covis_update_ref.py, which holds a real SetBadFlag on a copy of the observations.

Without a device: the exported symbols (they fail without the feature), the struct layout against the
stand-alone program's output, every ORBGPU_ERR_ARG cause, the stand-alone host program under the address and
undefined-behaviour sanitizers (tests/cpp/covis_update_args_main.cpp, which makes the calls with valid
arguments), the properties of the restatement and a host model of the bytes an insertion may write.

No call here has arguments that pass the checks and a pointer that is not a real allocation: such a call is a
launch on a machine that has a device.  The Python argument test only makes calls that are refused or have n ==
0; on the GPU every buffer is a torch allocation.

GPU: every comparison is exact -- integers and copied bytes, no tolerance anywhere.  The table is filled with
guard bytes before the rows are uploaded: below a count every entry equals the restatement's, and from
max(old count, new count) on every byte is the one that was there.
"""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import covis_ref as cr
import covis_update_ref as cur
import test_covis as tc

ROOT = Path(__file__).resolve().parent.parent
ROWS = (("conn", "n_conn", "conn_kf", "conn_w"), ("ord", "n_ord", "ord_kf", "ord_w"))
RESULT_KEYS = ("status", "n_counted", "n_ordered", "kf_max", "w_max", "front")


# ---- scenes ------------------------------------------------------------------------------------------------

def shared(S, a, b, w, **kw):
    """w points that a and b both see"""
    for _ in range(w):
        p = S.point()
        S.see(a, p, **kw)
        S.see(b, p, **kw)


def star(n_kf, x, weights, kf_by_rank=None):
    """keyframe x shares weights[nb] points with each keyframe nb"""
    S = cur.Scene(n_kf, kf_by_rank)
    for nb, w in weights.items():
        shared(S, x, nb, w)
    return S


def seen_by(S, k, others, n, octave=0, other_octave=0, **kw):
    """n points in keyframe k's slots that the keyframes `others` see too; returns them"""
    pts = []
    for _ in range(n):
        p = S.point()
        S.see(k, p, octave=octave, **kw)
        for o in others:
            S.see(o, p, octave=other_octave)
        pts.append(p)
    return pts


def culling_scene():
    """10 keyframes, 50 points: the list of `cur` is [A, first, B, E].  A is redundant.  Every point of B is seen by
    B, A, C and D: redundant while A observes it (nObs 4, three others), not once A is erased (nObs 3) -- B flips
    from culled to kept.  E holds 9 redundant points and one that only E and A see: with A erased that point is
    bad (nObs 1), nMPs drops from 10 to 9 and 9 > 0.9 * 9 -- E flips from kept to culled."""
    first, now, A, B, C, D, E, F, G, H = range(10)
    S = cur.Scene(10)
    S.first[first] = 1
    seen_by(S, A, (F, G, H), 10)
    seen_by(S, B, (A, C, D), 10)
    seen_by(S, E, (F, G, H), 9)
    seen_by(S, E, (A,), 1)
    seen_by(S, first, (F, G, H, C), 10)  # redundant, and never judged (:816)
    seen_by(S, now, (C, D), 10)
    S.slot(A)  # NULL
    S.see(A, S.point(valid=False))  # bad
    T = cr.Table(10, 8, ord={now: [(A, 40), (first, 30), (B, 20), (E, 10)]})
    return S, T, dict(now=now, A=A, B=B, E=E, first=first)


# ---- CPU: the restatement --------------------------------------------------------------------------------

def test_update_connections_in_the_restatement():
    """passes without the feature: it asserts on the restatement.  The ord row of UpdateConnections holds only the
    counts from 15 on, so it is not the best-covisibles of its conn row when a count is below 15"""
    S = star(6, 0, {1: 14, 2: 15, 3: 16, 4: 15})
    T = cr.Table(6, 8)
    r, = cur.update_connections(T, S, [0])
    assert r == dict(status=cur.OK, n_counted=4, n_ordered=3, kf_max=3, w_max=16, front=3)
    assert T.conn[0] == [(1, 14), (2, 15), (3, 16), (4, 15)]
    assert T.ord[0] == [(3, 16), (4, 15), (2, 15)] != cr.best_covisibles(T.conn[0])  # ties in descending rank
    assert T.conn[2] == [(0, 15)] and T.conn[1] == []  # AddConnection runs on the ordered set only
    # all below 15: the first strict maximum in rank order, alone
    S = star(5, 0, {1: 9, 2: 14, 3: 14})
    T = cr.Table(5, 8)
    r, = cur.update_connections(T, S, [0])
    assert (r["kf_max"], r["n_ordered"], T.ord[0], T.conn[2], T.conn[3]) == (2, 1, [(2, 14)], [(0, 14)], [])
    S.kf_by_rank = [4, 3, 2, 1, 0]
    T = cr.Table(5, 8)
    r, = cur.update_connections(T, S, [0])
    assert (r["kf_max"], T.ord[0], T.conn[0]) == (3, [(3, 14)], [(3, 14), (2, 14), (1, 9)])


def test_culling_in_the_restatement():
    """passes without the feature: culling one keyframe turns a point of few observations bad and changes later
    verdicts, in both directions"""
    S, T, nm = culling_scene()
    res, rows, culled = cur.keyframe_culling(T, S, nm["now"], mono=True)
    alone = cur.keyframe_culling(T, S, nm["now"], mono=True, set_bad=False)[1]
    A, B, E = nm["A"], nm["B"], nm["E"]
    assert alone == [(A, 21, 20, cur.CULLED), (nm["first"], 0, 0, cur.SKIPPED_FIRST), (B, 10, 10, cur.CULLED), (E, 10, 9, cur.KEPT)]
    assert rows == [(A, 21, 20, cur.CULLED), (nm["first"], 0, 0, cur.SKIPPED_FIRST), (B, 10, 0, cur.KEPT), (E, 9, 9, cur.CULLED)]
    assert culled == [A, E] and res == dict(status=cur.OK, n_list=4, n_culled=2, n_to_be_erased=0)
    L = cur.LiveMap(S)
    lone = S.slots[E][9]
    assert L.n_obs[lone] == 2 and not L.bad[lone]
    L.set_bad_flag(A)
    assert L.bad[lone] and L.slots[E][9] == -1 and L.n_obs[S.slots[B][0]] == 3
    S.not_erase[A] = 1  # mbNotErase: nothing changes, the later verdicts are those of the map as it stands
    res, rows, culled = cur.keyframe_culling(T, S, nm["now"], mono=True)
    assert rows == [(A, 21, 20, cur.TO_BE_ERASED)] + alone[1:] and culled == [B] and res["n_to_be_erased"] == 1


class HostUpdate(tc.HostGraph):
    """tc.HostGraph with the writes of csrc/covis.hip's update_apply_kernel: the insertion that moves [place, n) one
    place up and so writes the entry at the old count, the rank that writes the entries below the new count
    only, the keyframe's own rows up to their new counts -- so that what assert_rows asks of the bytes past the
    counts is checked without a device."""

    def update(self, T, S, kfs):
        h, rank_of, out = self.h, S.rank_of(), []
        for x in kfs:
            r, = cur.update_connections(T, S, [x])
            out.append(r)
            if r["status"] != cur.OK:
                continue
            for nb, w in T.ord[x]:
                n = int(h["n_conn"][nb])
                at = [i for i in range(n) if h["conn_kf"][nb, i] == x]
                if at and h["conn_w"][nb, at[0]] == w:
                    continue
                if at:
                    h["conn_w"][nb, at[0]] = w
                else:
                    place = sum(1 for i in range(n) if rank_of[int(h["conn_kf"][nb, i])] < rank_of[x])
                    for a in ("conn_kf", "conn_w"):
                        h[a][nb, place + 1:n + 1] = h[a][nb, place:n].copy()
                    h["conn_kf"][nb, place], h["conn_w"][nb, place] = x, w
                    n += 1
                h["n_conn"][nb] = h["n_ord"][nb] = n
                keys = sorted(((int(h["conn_w"][nb, i]), i) for i in range(n)), reverse=True)
                for q, (wq, i) in enumerate(keys):
                    h["ord_kf"][nb, q], h["ord_w"][nb, q] = h["conn_kf"][nb, i], wq
                best = [int(v) for v in h["ord_kf"][nb, :min(n, 10)]]
                h["covis10"][nb] = best + [-1] * (10 - len(best))
            for rows, cnt, a, b in ((T.conn[x], "n_conn", "conn_kf", "conn_w"), (T.ord[x], "n_ord", "ord_kf", "ord_w")):
                h[cnt][x] = len(rows)
                for i, (kf, w) in enumerate(rows):
                    h[a][x, i], h[b][x, i] = kf, w
            h["covis10"][x] = T.covis10(x)
        return out


def assert_rows(G, before, T, where, erased=False):
    """the table against the restatement's: the counts, every entry below them and the best 10; from max(old
    count, new count) of a row on, the bytes that were there before the call.  erased: after the erasure, which
    rebuilds an ord row from the whole conn row -- on a row that UpdateConnections left shorter than its conn row
    every rebuild may write up to the conn row's count, so the bound is the larger of the row's two old counts"""
    h = G.download()
    for k in range(T.n_kf):
        for name, cnt, a, b in ROWS:
            rows = getattr(T, name)[k]
            n, top = len(rows), max(len(rows), int(before[cnt][k]))
            if erased:
                top = max(top, int(before["n_conn"][k]))
            assert h[cnt][k] == n, (where, k, cnt)
            assert h[a][k, :n].tolist() == [kf for kf, _ in rows] and h[b][k, :n].tolist() == [w for _, w in rows], (where, k, a)
            assert h[a][k, top:].tobytes() == before[a][k, top:].tobytes() and h[b][k, top:].tobytes() == before[b][k, top:].tobytes(), (where, k, a)
        assert h["covis10"][k].tolist() == T.covis10(k), (where, k)


def add_three_ways():
    """x = 0 has the neighbours 1 (no row entry for 0), 2 (holds 0 with the weight it is about to get, and a
    hand-made stale ord row), 3 (holds 0 with another weight) and 5 (below 15: not touched)"""
    S = star(8, 0, {1: 15, 2: 16, 3: 17, 5: 3})
    conn = {1: [(4, 30), (6, 2)], 2: [(0, 16), (4, 9)], 3: [(0, 5), (6, 40), (7, 17)], 5: [(4, 1)]}
    T = cr.Table(8, 8, conn, ord={2: [(4, 9), (0, 16)]})  # stale: UpdateBestCovisibles would put 0 first
    return S, T


def test_bytes_past_the_counts_in_a_host_model_of_the_kernel():
    """passes without the feature: the kernel's writes restated on the host, through the same assert_rows as the
    GPU tests"""
    for S, T, kfs in (add_three_ways() + ([0],), (star(6, 0, {1: 14, 2: 15, 3: 16, 4: 15}), cr.Table(6, 8), [0, 2, 0]),
                      mutual() + ([0, 1],), mutual() + ([1, 0],)):
        G = HostUpdate(T)
        before = G.download()
        G.update(T, S, kfs)
        assert_rows(G, before, T, kfs)
    S, T = add_three_ways()
    G = HostUpdate(T)
    G.update(T, S, [0])
    assert G.h["ord_kf"][2, :2].tolist() == [4, 0] and T.ord[2] == [(4, 9), (0, 16)]  # equal weight: the stale row stays
    assert T.conn[1] == [(0, 15), (4, 30), (6, 2)] and T.ord[3] == [(6, 40), (7, 17), (0, 17)]
    assert G.h["conn_kf"][1, 3] == G.h["conn_kf"][4, 7]  # past the new count of 3: the guard


def mutual():
    """0 and 1 are each other's neighbours with unequal counts: 0 holds one shared point in two slots, so 0 counts
    21 and 1 counts 20.  The later job overwrites the earlier one's weight and rebuilds its ord row from the
    whole conn row, which holds the weak neighbour too: the two list orders leave different tables"""
    S = cur.Scene(5)
    shared(S, 0, 1, 20)
    S.slot(0, S.slots[0][0])
    shared(S, 0, 2, 5)
    shared(S, 1, 3, 6)
    return S, cr.Table(5, 4)


def test_list_order_matters_in_the_restatement():
    """passes without the feature"""
    S, Ta = mutual()
    _, Tb = mutual()
    cur.update_connections(Ta, S, [0, 1])
    cur.update_connections(Tb, S, [1, 0])
    assert Ta.conn[0] == [(1, 20), (2, 5)] and Ta.ord[0] == [(1, 20), (2, 5)] and Ta.ord[1] == [(0, 20)]
    assert Tb.conn[0] == [(1, 21), (2, 5)] and Tb.ord[0] == [(1, 21)] and Tb.ord[1] == [(0, 21), (3, 6)]


def test_looping_scene_culls_and_flips():
    """passes without the feature: the seed of the GPU test's random scene makes the restatement cull at least two
    keyframes and change at least one later verdict"""
    S, T = looping()
    rows = cur.keyframe_culling(T, S, LOOP_KF, mono=False)[1]
    alone = cur.keyframe_culling(T, S, LOOP_KF, mono=False, set_bad=False)[1]
    assert sum(r[3] == cur.CULLED for r in rows) >= 2
    assert sum(a[3] != b[3] for a, b in zip(rows, alone)) >= 1 and len(rows) > 20


LOOP_N, LOOP_KF, LOOP_SEED = 130, 129, 3
_LOOP = []


def looping():
    if not _LOOP:
        _LOOP.append(cur.looping_scene(LOOP_N, LOOP_SEED))
    S, T = _LOOP[0]
    return S, cr.Table(T.n_kf, T.stride, dict(enumerate(T.conn)), dict(enumerate(T.ord)))


# ---- without a GPU: the entry points' host side -------------------------------------------------------------

def test_library_has_the_update_connections_entry_point():
    """fails without the feature: the library has no such symbol"""
    import orbgpu
    assert hasattr(orbgpu.lib(), "orbgpu_covis_update_connections_batch_device")
    assert hasattr(orbgpu.lib(), "orbgpu_covis_update_workspace_bytes")


def test_library_has_the_keyframe_culling_entry_point():
    """fails without the feature: the library has no such symbol"""
    import orbgpu
    assert hasattr(orbgpu.lib(), "orbgpu_covis_keyframe_culling_batch_device")


def test_argument_errors_come_before_the_device():
    """every call here is refused or has n == 0: one with valid arguments would be launched on a machine that has a
    device, on pointers that are not memory; tests/cpp/covis_update_args_main.cpp makes those, on real arrays"""
    import covis
    import localba
    import track
    L = covis._lib()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused, or has nothing to do

    def filled(cls, skip=(), **kw):
        s = cls()
        for name, t in cls._fields_:
            if t is ctypes.c_void_p and name not in skip:
                setattr(s, name, 256)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    graph = lambda **kw: ctypes.byref(filled(covis.CovisGraphStruct, **dict(dict(n_kf=2, conn_stride=8), **kw)))
    counts = dict(n_kf=2, n_pt=3, n_slots_total=4, n_obs_total=5)
    mirror = lambda **kw: ctypes.byref(filled(track.MapMirrorStruct, **dict(counts, **kw)))
    ba = lambda **kw: ctypes.byref(filled(localba.MapMirrorBAStruct, **kw))
    cull = lambda **kw: ctypes.byref(filled(covis.MapMirrorCullStruct, **kw))
    need = L.orbgpu_covis_update_workspace_bytes(1, 2)
    assert need == 4 * (2 + 1 + 1 + 2) and L.orbgpu_covis_update_workspace_bytes(-1, 2) == 0
    assert L.orbgpu_covis_update_workspace_bytes(1 << 16, 1 << 16) == 0

    def update(n=1, kfs=p, m=None, g=None, ws=p, ws_bytes=need, res=p):
        return L.orbgpu_covis_update_connections_batch_device(n, kfs, m if m is not None else mirror(), g if g is not None else graph(),
                                                              ws, ws_bytes, res, None)

    read = ("slot_offset", "n_slots", "slots", "pt_flags", "obs_offset", "n_obs", "obs")
    bad = [dict(n=-1), dict(kfs=None), dict(res=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
           dict(g=graph(n_kf=3)), dict(m=mirror(n_kf=3)), dict(g=graph(conn_stride=0)), dict(g=graph(conn_stride=covis.MAX_STRIDE + 1)),
           dict(g=graph(n_kf=-1), m=mirror(n_kf=-1)), dict(g=graph(n_kf=1 << 29), m=mirror(n_kf=1 << 29))]
    bad += [dict(m=mirror(**{k: -1})) for k in ("n_pt", "n_slots_total", "n_obs_total")]
    bad += [dict(m=mirror(**{k: None})) for k in read]
    bad += [dict(g=graph(**{k: None})) for k, _ in covis.CovisGraphStruct._fields_[2:]]
    for kw in bad:
        assert update(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    fn = L.orbgpu_covis_update_connections_batch_device
    assert fn(1, p, None, graph(), p, need, p, None) == -1 and fn(1, p, mirror(), None, p, need, p, None) == -1
    assert fn(0, None, None, None, None, 0, None, None) == 0
    assert fn(0, None, mirror(), graph(), None, 0, None, None) == 0
    assert fn(0, None, mirror(), graph(n_kf=3), None, 0, None, None) == -1  # what is given is checked

    def culling(n=1, jobs=p, m=None, b=None, c=None, g=None, list_stride=8, res=p, verdicts=p, culled=p):
        return L.orbgpu_covis_keyframe_culling_batch_device(n, jobs, m if m is not None else mirror(), b if b is not None else ba(),
                                                            c if c is not None else cull(), g if g is not None else graph(),
                                                            list_stride, res, verdicts, culled, None)

    bad = [dict(n=-1), dict(jobs=None), dict(res=None), dict(verdicts=None), dict(culled=None), dict(list_stride=0),
           dict(list_stride=-4), dict(n=1 << 20, list_stride=1 << 20), dict(g=graph(n_kf=3)), dict(g=graph(conn_stride=0)),
           dict(m=mirror(n_obs_total=-1))]
    bad += [dict(m=mirror(**{k: None})) for k in read]
    bad += [dict(b=ba(**{k: None})) for k in ("kf_first", "kp_obs", "obs_idx")]
    bad += [dict(c=cull(**{k: None})) for k, _ in covis.MapMirrorCullStruct._fields_]
    bad += [dict(g=graph(**{k: None})) for k, _ in covis.CovisGraphStruct._fields_[2:]]
    for kw in bad:
        assert culling(**kw) == -1, kw
    fn = L.orbgpu_covis_keyframe_culling_batch_device
    for args in ((None, ba(), cull(), graph()), (mirror(), None, cull(), graph()), (mirror(), ba(), None, graph()),
                 (mirror(), ba(), cull(), None)):
        assert fn(1, p, *args, 8, p, p, p, None) == -1
    assert fn(0, None, None, None, None, None, 1, None, None, None, None) == 0
    assert fn(0, None, mirror(), ba(), cull(), graph(), 8, None, None, None, None) == 0
    assert fn(0, None, mirror(), ba(), cull(kp_depth=None), graph(), 8, None, None, None, None) == -1


@pytest.fixture(scope="module")
def args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("covis_update_args") / "covis_update_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "covis_update_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(args_main):
    """the calls with valid arguments (ORBGPU_ERR_NO_DEVICE: the device check is stubbed) and the argument checks,
    compiled for the host with -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layouts_equal_the_header(args_main):
    import covis
    r = subprocess.run([str(args_main), "sizes"], capture_output=True, text=True, check=True)
    got = {k: int(v) for k, v in re.findall(r"(\S+) (\d+)", r.stdout)}
    want = {}
    for prefix, cls, name in (("update_result", covis.UpdateResult, "orbgpu_covis_update_result"),
                              ("mirror_cull", covis.MapMirrorCullStruct, "orbgpu_map_mirror_cull"),
                              ("cull_job", covis.CullJob, "orbgpu_covis_cull_job"),
                              ("cull_verdict", covis.CullVerdict, "orbgpu_covis_cull_verdict"),
                              ("cull_result", covis.CullResult, "orbgpu_covis_cull_result")):
        want[name] = ctypes.sizeof(cls)
        for f, _ in cls._fields_[1:]:
            if f != "pad":
                want[f"{prefix}.{f}"] = getattr(cls, f).offset
    want.update({"status.EMPTY": covis.EMPTY, "status.CAPACITY": covis.CAPACITY, "verdict.KEPT": covis.KEPT,
                 "verdict.CULLED": covis.CULLED, "verdict.TO_BE_ERASED": covis.TO_BE_ERASED,
                 "verdict.SKIPPED_FIRST": covis.SKIPPED_FIRST, "th": covis.TH})
    assert got == want
    assert (covis.OK, covis.EMPTY, covis.CAPACITY, covis.BAD_JOB) == (cur.OK, cur.EMPTY, cur.CAPACITY, cur.BAD_JOB)
    assert (covis.KEPT, covis.CULLED, covis.TO_BE_ERASED, covis.SKIPPED_FIRST) == (cur.KEPT, cur.CULLED, cur.TO_BE_ERASED, cur.SKIPPED_FIRST)
    assert covis.TH == cur.TH and covis.UPDATE_RESULT_DTYPE.fields["front"][1] == covis.UpdateResult.front.offset


# ---- GPU ----------------------------------------------------------------------------------------------

def to_device(S):
    """the Scene as the three mirrors in HBM"""
    import covis
    import localba
    import track
    n_kf, n_pt = S.n_kf, len(S.pt_valid)
    z = lambda *shape: np.zeros(shape, np.float32)
    mirror = track.MapMirror(
        kf_bad=np.zeros(n_kf, np.uint8), slots=[np.array(s, np.int32) for s in S.slots], covis=np.full((n_kf, 10), -1, np.int32),
        children=[[] for _ in range(n_kf)], parent=np.full(n_kf, -1, np.int32),
        pt_flags=np.array([(1 if v else 0) | (2 if o else 0) for v, o in zip(S.pt_valid, S.obs)], np.int32), obs=S.obs,
        pos=z(n_pt, 3), normal=z(n_pt, 3), desc=np.zeros((n_pt, 32), np.uint8), min_dist=z(n_pt), max_dist=z(n_pt),
        kf_by_rank=S.kf_by_rank)
    kp_obs = [np.array([(0.0, 0.0, 7.5 if st else -1.0) for st in row], np.float32).reshape(-1, 3) for row in S.stereo]
    mirror_ba = localba.MapMirrorBA(covis_all=[[] for _ in range(n_kf)], kf_first=np.array(S.first, np.uint8), kf_Tcw=z(n_kf, 12),
                                    kf_cam=z(n_kf, 5), kp_obs=kp_obs, kp_inv_sigma2=[np.ones(len(r), np.float32) for r in S.stereo],
                                    obs_idx=S.idx)
    cull = covis.MapMirrorCull(S.octave, S.depth, np.array(S.th_depth, np.float32), np.array(S.not_erase, np.uint8))
    return mirror, mirror_ba, cull


def assert_results(res, want, where):
    assert len(res) == len(want), where
    for i, w in enumerate(want):
        assert {k: int(res[k][i]) for k in RESULT_KEYS} == w, (where, i)
        assert res["pad"][i].tolist() == [0, 0]


def run_update(torch, S, T, kfs, ref=None, mirror=None):
    """UpdateConnections of `kfs` in one call on a guard-filled table that holds T; compares the results and the
    table with the restatement, run on ref = (scene, list) when the device's mirror was tampered with"""
    import covis
    mirror = mirror or to_device(S)[0]
    G = tc.make_graph(torch, T)
    before = G.download()
    res = covis.update_results(covis.update_connections(G, mirror, kfs))
    want = cur.update_connections(T, *(ref or (S, kfs)))
    assert_results(res, want, kfs)
    assert_rows(G, before, T, kfs)
    return G, res, before


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [1, 63, 64, 65, 1030])
def test_gpu_update_slot_counts(n_slots):
    """a keyframe of 1, 63, 64 and 65 slots, and of more than one round of the counting workgroups; below 15 the one
    neighbour is the single maximum"""
    torch = tc._gpu()
    S = star(3, 1, {2: n_slots})
    _, res, _ = run_update(torch, S, cr.Table(3, 4), [1])
    assert (int(res["w_max"][0]), int(res["n_ordered"][0]), int(res["front"][0])) == (n_slots, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_counted", [1, 64, 65])
def test_gpu_update_counted_keyframes_and_capacity(n_counted):
    """1, 64 and 65 counted keyframes in rows of 64: 65 is CAPACITY and the table keeps every byte.  The counted
    keyframes lie beyond index 1024, past the first round of the walk in rank order"""
    torch = tc._gpu()
    n_kf = 1100
    S = star(n_kf, 3, {1030 + i: 1 + (i % 3 == 1) for i in range(n_counted)})
    T = cr.Table(n_kf, 64, {1030: [(7, 3)]})
    G, res, before = run_update(torch, S, T, [3])
    assert int(res["status"][0]) == (cur.CAPACITY if n_counted == 65 else cur.OK) and int(res["n_counted"][0]) == n_counted
    assert int(res["kf_max"][0]) == (1031 if n_counted > 1 else 1030)
    if n_counted == 65:
        h = G.download()
        assert all(h[k].tobytes() == before[k].tobytes() for k in h)


@pytest.mark.gpu
def test_gpu_update_full_neighbour_is_capacity():
    """a neighbour that needs an insertion and holds conn_stride entries: CAPACITY, decided before the first write
    (the other neighbour, which has room, is not written either).  A full neighbour that already holds the key
    is no obstacle"""
    torch = tc._gpu()
    S = star(12, 0, {1: 20, 2: 15})
    full = [(k, 3) for k in range(3, 7)]
    T = cr.Table(12, 4, {2: full})
    G, res, before = run_update(torch, S, T, [0])
    h = G.download()
    assert int(res["status"][0]) == cur.CAPACITY and all(h[k].tobytes() == before[k].tobytes() for k in h)
    T = cr.Table(12, 4, {2: [(0, 9)] + full[1:]})
    _, res, _ = run_update(torch, S, T, [0])
    assert int(res["status"][0]) == cur.OK and T.conn[2][0] == (0, 15)


@pytest.mark.gpu
def test_gpu_update_threshold_ties_and_fallback():
    """counts of 14, 15 and 16; equal weights in the ordered set (ties in descending rank); all below 15 with two
    equal maxima (the first strict maximum in rank order, alone); a duplicate point in two slots that lifts 14 to
    15; -1 slots and bad points; an empty counter"""
    torch = tc._gpu()
    S = star(8, 0, {1: 14, 2: 15, 3: 16, 4: 15, 6: 16})
    _, res, _ = run_update(torch, S, cr.Table(8, 8), [0])
    assert (int(res["n_counted"][0]), int(res["n_ordered"][0]), int(res["kf_max"][0]), int(res["front"][0])) == (5, 4, 3, 6)
    S = star(5, 0, {1: 9, 2: 14, 3: 14})
    T = cr.Table(5, 8)
    _, res, _ = run_update(torch, S, T, [0])
    assert int(res["kf_max"][0]) == 2 and T.ord[0] == [(2, 14)] and T.conn[3] == []
    S.slot(0, S.slots[0][-1])  # the last point shared with 3, held twice: 3 counts 15
    S.slot(0)
    S.see(0, S.point(valid=False))
    S.see(4, S.slots[0][-1])  # a bad point's observers are not counted
    T = cr.Table(5, 8)
    _, res, _ = run_update(torch, S, T, [0])
    assert T.ord[0] == [(3, 15)] and T.conn[0] == [(1, 9), (2, 14), (3, 15)] and T.conn[4] == []
    E = cur.Scene(3)
    E.slot(1)
    E.see(1, E.point())
    E.see(1, E.point(valid=False))
    E.see(2, E.slots[1][2])
    T = cr.Table(3, 4, {1: [(0, 5)]})
    G, res, before = run_update(torch, E, T, [1, 0])
    assert res["status"].tolist() == [cur.EMPTY, cur.EMPTY] and T.conn[1] == [(0, 5)]
    h = G.download()
    assert all(h[k].tobytes() == before[k].tobytes() for k in h)


@pytest.mark.gpu
def test_gpu_update_rank_order():
    """kf_by_rank NULL, and a permutation for which the rows, the maximum and the ties differ from ascending index;
    an insertion goes to its rank position in the neighbour's row"""
    torch = tc._gpu()
    weights = {1: 20, 2: 14, 3: 20, 4: 3, 5: 14}
    perm = [4, 5, 3, 0, 1, 2]
    tables = []
    for rank in (None, perm):
        S = star(6, 0, weights, rank)
        order = list(range(6)) if rank is None else rank
        rows = {k: [(q, 30 + q) for q in order if q not in (0, k)][:3] for k in (1, 3)}
        T = cr.Table(6, 8, rows)
        run_update(torch, S, T, [0])
        tables.append((T.conn, T.ord))
    assert tables[0] != tables[1]
    assert tables[0][1][0] == [(3, 20), (1, 20)] and tables[1][1][0] == [(1, 20), (3, 20)]
    assert [k for k, _ in tables[1][0][1]] == [4, 5, 3, 0] and [k for k, _ in tables[0][0][1]] == [0, 2, 3, 4]
    S = star(5, 0, {1: 9, 2: 14, 3: 14}, [4, 3, 2, 1, 0])
    _, res, _ = run_update(torch, S, cr.Table(5, 8), [0])
    assert int(res["kf_max"][0]) == 3


@pytest.mark.gpu
def test_gpu_update_add_connection_three_ways():
    """the key absent (inserted, the neighbour's rows rebuilt), held with an equal weight (nothing happens: a
    hand-made stale ord row stays stale) and held with another weight (overwritten, rebuilt)"""
    torch = tc._gpu()
    S, T = add_three_ways()
    G, _, _ = run_update(torch, S, T, [0])
    assert T.ord[2] == [(4, 9), (0, 16)] and T.conn[1] == [(0, 15), (4, 30), (6, 2)] and T.ord[3] == [(6, 40), (7, 17), (0, 17)]
    assert T.conn[5] == [(4, 1)] and G.lists() == (T.conn, T.ord)


@pytest.mark.gpu
def test_gpu_update_batch_follows_the_list_order():
    """two jobs that are each other's neighbours, in both list orders, with different final tables; the batch equals
    one call per job with the table carried along; a repeat run gives the same bytes"""
    torch = tc._gpu()
    import covis
    got = []
    for kfs in ([0, 1], [1, 0]):
        S, T = mutual()
        G, _, _ = run_update(torch, S, T, kfs)
        got.append(G.download())
        S, T1 = mutual()
        mirror = to_device(S)[0]
        G1 = tc.make_graph(torch, T1)
        for k in kfs:
            covis.update_connections(G1, mirror, [k])
        one = G1.download()
        assert all(one[name].tobytes() == got[-1][name].tobytes() for name in one)
        G2, _, _ = run_update(torch, *mutual(), kfs)
        again = G2.download()
        assert all(again[name].tobytes() == got[-1][name].tobytes() for name in again)
    assert got[0]["conn_w"][0, 0] == 20 and got[1]["conn_w"][0, 0] == 21 and got[0]["n_ord"][0] == 2 and got[1]["n_ord"][0] == 1


def bad_scene():
    """keyframes 0 and 6 are good jobs; 1 holds a point id beyond the map, 2 a point id below -1, 3 a point with an
    observer beyond the map, 4 and 5 are good until the device's mirror is tampered with"""
    S = cur.Scene(8)
    shared(S, 0, 7, 16)
    shared(S, 6, 7, 15)
    shared(S, 6, 0, 2)
    for k in (1, 2, 3, 4, 5):
        shared(S, k, 7, 15)
    p = S.point()
    S.see(3, p)
    S.obs[p].append(8)
    S.idx[p].append(0)
    S.slot(1, len(S.pt_valid))
    S.slot(2, -2)
    return S


@pytest.mark.gpu
def test_gpu_update_bad_jobs_between_good_ones():
    """every BAD_JOB cause between good jobs: a keyframe index, a point id, an observer, a slot range and an
    observation range outside the mirror.  Such a job writes its result only; a kf_by_rank entry outside the
    mirror makes every job one"""
    torch = tc._gpu()
    S = bad_scene()
    kfs = [0, -1, 1, 8, 2, 3, 6]
    _, res, _ = run_update(torch, S, cr.Table(8, 8), kfs)
    assert res["status"].tolist() == [0, 3, 3, 3, 3, 3, 0]
    mirror = to_device(S)[0]
    mirror.t["n_slots"].view(torch.int32)[4] = 1 << 20  # slot_offset + n_slots beyond slots[]
    p = S.slots[5][3]
    mirror.t["obs_offset"].view(torch.int32)[p] = -4
    _, res, _ = run_update(torch, S, cr.Table(8, 8), [0, 4, 5, 6], ref=(S, [0, -1, -1, 6]), mirror=mirror)
    assert res["status"].tolist() == [0, 3, 3, 0]
    mirror = to_device(S)[0]
    mirror.t["n_obs"].view(torch.int32)[S.slots[0][0]] = 1 << 30  # obs_offset + n_obs beyond obs[]
    run_update(torch, S, cr.Table(8, 8), [6, 0], ref=(S, [6, -1]), mirror=mirror)
    S.kf_by_rank = [0, 1, 2, 3, 8, 5, 6, 7]
    mirror = to_device(S)[0]
    S.kf_by_rank = None
    _, res, _ = run_update(torch, S, cr.Table(8, 8), [0, 6], ref=(S, [-1, -1]), mirror=mirror)
    assert res["status"].tolist() == [3, 3]


def scene_of_mirror(m):
    """a localba_map_scene mirror as a Scene for the restatement (what UpdateConnections reads of it)"""
    S = cur.Scene(len(m["kf_bad"]), m["kf_by_rank"])
    S.slots = [[int(p) for p in s] for s in m["slots"]]
    S.pt_valid = [bool(f & 1) for f in m["pt_flags"]]
    S.obs = [list(o) for o in m["obs"]]
    return S


@pytest.mark.gpu
def test_gpu_update_then_the_gather_reads_the_rows_in_place():
    """covis_all pointed at the table with CovisGraph.attach: after UpdateConnections of pKF on the same stream the
    LBA gather's outputs equal the gather on host-built lists from the restatement's table"""
    torch = tc._gpu()
    import covis
    import localba
    import localba_map_ref as lr
    import localba_map_scene as ls
    import test_localba_map as tm
    import track
    sc = ls.SCENES["rich"]()
    nm, n_kf = sc["names"], len(sc["mirror"]["kf_bad"])
    a = nm["a"]
    S = scene_of_mirror(sc["mirror"])
    T = cr.Table(n_kf, 8, {k: sorted((int(c), 100 - i) for i, c in enumerate(lst)) for k, lst in enumerate(sc["ba"]["covis_all"]) if k != a})
    mirror, mirror_ba = track.MapMirror(**sc["mirror"]), localba.MapMirrorBA(**sc["ba"])
    G = tc.make_graph(torch, T, covis10=mirror.t["covis"])
    G.attach(mirror_ba)
    before = G.download()
    B = localba.MapLocalBA(mirror, mirror_ba, [a], **tm.BIG)
    tm.guard_fill(torch, B)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    results = covis.update_connections(G, mirror, [a], stream=stream)
    B.gather(stream)
    stream.synchronize()
    want_res = cur.update_connections(T, S, [a])
    assert_results(covis.update_results(results), want_res, "pKF")
    assert_rows(G, before, T, "pKF")
    assert want_res[0]["status"] == cur.OK and len(T.conn[a]) > len(T.ord[a]) == 1  # every count is below 15
    listed = dict(sc["ba"], covis_all=[[k for k, _ in T.ord[i]] for i in range(n_kf)])
    want = lr.gather(sc["mirror"], listed, a, **tm.BIG)
    assert want.status == lr.OK and want.local_kfs[0] == a
    B.h = {name: B.host(name) for name in B.t if name not in ("gather_ws", "gather_jobs")}
    tm.assert_job(B, 0, want, "gather after UpdateConnections")
    assert mirror.t["covis"].cpu().numpy().view(np.int32).reshape(n_kf, 10)[a].tolist() == T.covis10(a)


# ---- GPU: KeyFrameCulling ----------------------------------------------------------------------------------

def run_culling(torch, S, T, jobs, list_stride=None, dev=None):
    """the jobs (kf, mono) in one call on a guard-filled table that holds T, against the restatement run once per
    job; the graph keeps every byte.  Returns (the Culling, the graph, the restatement's per-job outputs)"""
    import covis
    dev = dev or to_device(S)
    G = tc.make_graph(torch, T)
    before = G.download()
    stride = list_stride or T.stride
    C = covis.keyframe_culling(G, *dev, jobs, list_stride=list_stride, guard=tc.GUARD)
    res, verdicts, culled = C.host()
    h = G.download()
    assert all(h[k].tobytes() == before[k].tobytes() for k in h)
    want = []
    for i, (kf, mono) in enumerate(jobs):
        w_res, w_rows, w_culled = cur.keyframe_culling(T, S, kf, bool(mono))
        want.append((w_res, w_rows, w_culled))
        if len(w_rows) > stride:
            w_res, w_rows, w_culled = dict(status=cur.CAPACITY, n_list=len(w_rows), n_culled=0, n_to_be_erased=0), [], []
        assert {k: int(res[k][i]) for k in w_res} == w_res and res["pad"][i].tolist() == [0] * 4, (jobs, i)
        assert [tuple(int(v) for v in row) for row in verdicts[i, :len(w_rows)].tolist()] == w_rows, (jobs, i)
        assert (verdicts[i, len(w_rows):].view(np.uint8) == tc.GUARD).all(), (jobs, i)  # past n_list: not written
        assert culled[i].tolist() == [r[0] if r[3] == cur.CULLED else -1 for r in w_rows] + [-1] * (stride - len(w_rows)), (jobs, i)
    return C, G, want


@pytest.mark.gpu
def test_gpu_culling_erasures_change_later_verdicts():
    """the hand-built scene: the first entry is culled and a later verdict flips in each direction -- a point that
    loses an observer drops to nObs 3, and a point that turns bad shrinks nMPs; the map's first keyframe in the
    list; then the same with mbNotErase on the first entry: TO_BE_ERASED, the later verdicts those of the map as
    it stands"""
    torch = tc._gpu()
    S, T, nm = culling_scene()
    _, _, want = run_culling(torch, S, T, [(nm["now"], 1)])
    assert [r[3] for r in want[0][1]] == [cur.CULLED, cur.SKIPPED_FIRST, cur.KEPT, cur.CULLED]
    S.not_erase[nm["A"]] = 1
    _, _, want = run_culling(torch, S, T, [(nm["now"], 1)])
    assert [r[3] for r in want[0][1]] == [cur.TO_BE_ERASED, cur.SKIPPED_FIRST, cur.CULLED, cur.KEPT]


def threshold_scene():
    """keyframes 1..4 with nMPs 10, 10, 20, 20 and 9, 10, 18, 19 redundant points: 9 > 0.9 * 10 and 18 > 0.9 * 20
    are false.  The other observers (5..8) are in no list.  Keyframes 9, 10: the octave rule, every point's
    three other observers at octave + 1 (redundant) and one of them at octave + 2 (not)"""
    S = cur.Scene(11)
    for k, n, red in ((1, 10, 9), (2, 10, 10), (3, 20, 18), (4, 20, 19)):
        seen_by(S, k, (5, 6, 7, 8), red)
        seen_by(S, k, (5, 6), n - red)
    seen_by(S, 9, (5, 6, 7), 10, octave=2, other_octave=3)
    for p in seen_by(S, 10, (5, 6), 10, octave=2, other_octave=3):
        S.see(7, p, octave=4)
    return S, cr.Table(11, 8, ord={0: [(k, 50 - k) for k in (1, 2, 3, 4, 9, 10)]})


@pytest.mark.gpu
def test_gpu_culling_ninety_percent_and_the_octave_rule():
    """(double)nRedundant > 0.9 * (double)nMPs at nMPs 10 and 20 with 9 / 10 and 18 / 19 redundant points, and the
    octave rule at octave + 1 and octave + 2"""
    torch = tc._gpu()
    S, T = threshold_scene()
    _, _, want = run_culling(torch, S, T, [(0, 1)])
    assert [r[1:] for r in want[0][1]] == [(10, 9, cur.KEPT), (10, 10, cur.CULLED), (20, 18, cur.KEPT), (20, 19, cur.CULLED),
                                           (10, 10, cur.CULLED), (10, 0, cur.KEPT)]


def stereo_scene():
    """K1 (stereo): 8 close redundant points and 2 far ones (and one of negative depth) that nobody else sees --
    kept when judged monocular (8 of 11), culled when stereo (8 of 8).  K2: 10 points seen by K1 (a stereo
    observation, 2 of nObs) and two monocular keyframes: nObs 5 and three others while K1 observes, nObs 3 once it
    is erased, which only the stereo judgement does.  K3: 10 points each seen by one other stereo keyframe: nObs 4
    but one other observer -- never redundant"""
    K1, K2, K3, X, Y, Z = 1, 2, 3, 4, 5, 6
    S = cur.Scene(7)
    seen_by(S, K1, (X, Y, Z), 8, stereo=True, depth=3.0)
    seen_by(S, K1, (), 2, stereo=True, depth=100.0)
    seen_by(S, K1, (), 1, stereo=False, depth=-1.0)
    for _ in range(10):
        p = S.point()
        S.see(K2, p, depth=2.0)
        S.see(K1, p, stereo=True, depth=2.0)
        S.see(X, p)
        S.see(Y, p)
        q = S.point()
        S.see(K3, q, stereo=True, depth=35.0)  # == mThDepth: not beyond it
        S.see(Z, q, stereo=True)
    return S, cr.Table(7, 8, ord={0: [(K1, 9), (K2, 8), (K3, 7)]})


@pytest.mark.gpu
def test_gpu_culling_stereo_and_monocular():
    """the depth tests and the 2-per-observation nObs, judged once monocular and once stereo in one call: two jobs
    with the same list that do not see each other's erasures"""
    torch = tc._gpu()
    S, T = stereo_scene()
    _, _, want = run_culling(torch, S, T, [(0, 1), (0, 0), (0, 1)])
    mono, stereo = want[0][1], want[1][1]
    assert [r[1:] for r in mono] == [(21, 18, cur.KEPT), (10, 10, cur.CULLED), (10, 0, cur.KEPT)]
    assert [r[1:] for r in stereo] == [(18, 18, cur.CULLED), (10, 0, cur.KEPT), (10, 0, cur.KEPT)]
    assert want[2] == want[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_list", [0, 1, 65])
def test_gpu_culling_list_lengths_and_capacity(n_list):
    """a list of 0, 1 and 65 entries; 65 entries in rows of 64 verdicts are CAPACITY: the result only, and culled all
    -1.  The judged keyframe has more slots than the workgroup has threads"""
    torch = tc._gpu()
    S = cur.Scene(70)
    for k in range(1, 1 + n_list):
        seen_by(S, k, (66, 67, 68), 1100 if k == 1 else 3)
        seen_by(S, k, (), k % 2)  # 3 of 4: not redundant enough (1100 of 1101 is)
    S.see(69, S.point())
    T = cr.Table(70, 65, ord={0: [(k, 200 - k) for k in range(1, 1 + n_list)]})
    _, _, want = run_culling(torch, S, T, [(0, 1)])
    assert want[0][0]["n_list"] == n_list and want[0][0]["n_culled"] == n_list // 2 + (n_list > 0)  # the even ones and 1
    if n_list == 65:
        C, _, _ = run_culling(torch, S, T, [(0, 1), (1, 1)], list_stride=64)
        res = C.host()[0]
        assert res["status"].tolist() == [cur.CAPACITY, cur.OK] and res["n_list"].tolist() == [65, 0]


@pytest.mark.gpu
def test_gpu_culling_bad_jobs():
    """a keyframe index, a list entry, a point id, an obs_idx, a slot range and an observation range outside the
    mirror: BAD_JOB, the result only and culled all -1, beside a good job"""
    torch = tc._gpu()
    import covis
    S, T, nm = culling_scene()
    T.ord[nm["B"]] = [(nm["A"], 5), (10, 4)]  # a list entry beyond the table
    S.slot(4, 999)
    T.ord[nm["E"]] = [(4, 3)]  # keyframe 4 (C) holds a point id beyond the map
    dev = to_device(S)
    G = tc.make_graph(torch, T)
    jobs = [(nm["now"], 1), (-1, 1), (10, 0), (nm["B"], 1), (nm["E"], 1)]
    C = covis.keyframe_culling(G, *dev, jobs)
    res, verdicts, culled = C.host()
    assert res["status"].tolist() == [cur.OK, cur.BAD_JOB, cur.BAD_JOB, cur.BAD_JOB, cur.BAD_JOB]
    assert res["n_culled"].tolist() == [2, 0, 0, 0, 0] and (culled[1:] == -1).all() and res["n_list"][1:].tolist() == [0] * 4
    S2, T2, _ = culling_scene()
    assert [tuple(r) for r in verdicts[0, :4].tolist()] == cur.keyframe_culling(T2, S2, nm["now"], True)[1]
    S2.idx[S2.slots[nm["A"]][0]][0] = 500  # an obs_idx beyond its keyframe's slots
    C = covis.keyframe_culling(tc.make_graph(torch, T2), *to_device(S2), [(nm["now"], 1)])
    assert C.host()[0]["status"].tolist() == [cur.BAD_JOB] and (C.host()[2] == -1).all()
    S3, T3, _ = culling_scene()
    for name, at, value in (("n_slots", nm["B"], 1 << 20), ("slot_offset", nm["E"], -8), ("n_obs", S3.slots[nm["E"]][0], 1 << 30)):
        dev = to_device(S3)  # a slot range and an observation range beyond their arrays
        dev[0].t[name].view(torch.int32)[at] = value
        C = covis.keyframe_culling(tc.make_graph(torch, T3), *dev, [(nm["now"], 1)], guard=tc.GUARD)
        res, verdicts, culled = C.host()
        assert res["status"].tolist() == [cur.BAD_JOB] and (culled == -1).all() and (verdicts.view(np.uint8) == tc.GUARD).all(), name


@pytest.mark.gpu
def test_gpu_culling_then_erasure_on_one_stream():
    """the chain culling -> erase on one stream with no download between them: the table equals the restatement's
    after its sequential SetBadFlags, and the erasure's statuses are OK exactly where a keyframe was culled"""
    torch = tc._gpu()
    import covis
    S, T = looping()
    stream = torch.cuda.Stream()
    dev = to_device(S)
    G = tc.make_graph(torch, T)
    before = G.download()
    torch.cuda.synchronize()
    C = covis.keyframe_culling(G, *dev, [(LOOP_KF, 0)], stream=stream)
    status = C.erase()
    stream.synchronize()
    res, rows, culled = cur.keyframe_culling(T, S, LOOP_KF, mono=False)
    assert len(culled) >= 2 and C.host()[2][0].tolist() == [r[0] if r[3] == cur.CULLED else -1 for r in rows] + [-1] * (T.stride - len(rows))
    assert cr.erase_keyframes(T, culled) == [cr.OK] * len(culled)
    assert status.cpu().numpy().tolist() == [cr.OK if r[3] == cur.CULLED else cr.BAD_JOB for r in rows] + [cr.BAD_JOB] * (T.stride - len(rows))
    assert_rows(G, before, T, "culling -> erase", erased=True)


@pytest.mark.gpu
def test_gpu_culling_random_looping_scene():
    """a random looping path of 130 keyframes, stereo and monocular keypoints mixed, against the restatement: at
    least two keyframes are culled and at least one later verdict is changed by the erasures; judged stereo and
    monocular, and for a second keyframe"""
    torch = tc._gpu()
    S, T = looping()
    _, _, want = run_culling(torch, S, T, [(LOOP_KF, 0), (LOOP_KF, 1), (LOOP_N // 2, 0)], dev=to_device(S))
    rows = want[0][1]
    alone = cur.keyframe_culling(T, S, LOOP_KF, mono=False, set_bad=False)[1]
    assert sum(r[3] == cur.CULLED for r in rows) >= 2 and sum(a[3] != b[3] for a, b in zip(rows, alone)) >= 1
