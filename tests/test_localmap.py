"""Tracking::UpdateLocalMap on the device (src/Tracking.cpp:1571-1745):
orbgpu_update_local_map_batch_device (include/orbgpu_localmap.h,
csrc/localmap.hip) against tests/localmap_ref.py on tests/localmap_scene.py's
constructed maps.

CPU: the restatement itself on every named scene -- the K2 walk around 80
members, the parent's break, bad neighbours / children / parents, the eleventh
covisible, child lists of 21 / 22 / 90, bad voted keyframes, ties under both orders, no votes, nulled held
points, first occurrences, extras, LAST_SEEN -- and its table fed to
track_ref.track_local against the table track_scene.chain_local builds by hand.
Without a device: the exported symbols (fails without the feature), argument
errors before the device, the stand-alone host program under the address and
undefined-behaviour sanitizers (tests/cpp/localmap_args_main.cpp), the struct
layouts.

GPU: every int of the result, local_kfs, local_points and frame_mp and every
byte of the filled table equal to the reference, with guard bytes past every
count intact; the edge sizes; initial -> update_local_map -> local_map on one
stream; independence of the batch, the position and the run; CAPACITY and
BAD_JOB jobs ending alone.  No tolerances: integers and copied bytes (the
chain's pose is held to tests/test_track.py's own bound by its own helper).
"""
import ctypes
import functools
import os
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import localmap_ref as lr
import localmap_scene as ls
import track_ref as tr
import track_scene as ts

ROOT = Path(__file__).resolve().parent.parent
S, P, KS = 320, 1024, 96  # stride, point_stride, kf_stride of the GPU runs unless a test says otherwise
GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def scene(name):
    return ls.SCENES[name]()


@functools.lru_cache(maxsize=None)
def ref(name, stride=S, point_stride=P, kf_stride=KS):
    sc = scene(name)
    return lr.update_local_map(sc["mirror"], sc["job"], stride, point_stride, kf_stride)


# ---- CPU: the K2 walk ---------------------------------------------------------------

@pytest.mark.parametrize("n,total,added", [(79, 81, 2), (80, 81, 1), (81, 81, 0), (82, 82, 0)])
def test_walk_stops_once_the_list_holds_more_than_80(n, total, added):
    """passes without the feature: it asserts on the restatement.  With 80 the first iteration still adds (80 is
    not > 80), with 81 none does."""
    sc, r = scene(f"k1_{n}"), ref(f"k1_{n}")
    assert (r.status, r.n_k1, r.n_local_kfs) == (lr.OK, n, total)
    assert r.local_kfs[:n] == sc["names"]["k1"] and r.local_kfs[n:] == sc["names"]["extra"][:added]
    assert r.n_local == n + 2 * added


def test_walk_parent_break_bad_ones_and_the_eleventh():
    """passes without the feature: it asserts on the restatement"""
    sc, r = scene("parent_break"), ref("parent_break")
    nm = sc["names"]  # the first member's neighbour, then its parent, and nothing of the later members
    assert r.local_kfs == nm["k1"] + [nm["first"], nm["parent"]] and not set(nm["later"]) & set(r.local_kfs)
    sc, r = scene("bad_ones"), ref("bad_ones")
    nm = sc["names"]
    assert r.local_kfs == [nm["a"]] + nm["added"] and sc["mirror"]["kf_bad"][nm["added"][2]] == 1
    assert not set(nm["bad"]) & set(r.local_kfs) and nm["never"] not in r.local_kfs
    sc, r = scene("eleventh"), ref("eleventh")
    assert r.local_kfs == sc["names"]["k1"] and sc["names"]["late"] not in r.local_kfs and r.n_k1 == 4


# ---- CPU: the votes -------------------------------------------------------------------

def test_votes_bad_keyframes_ties_and_none():
    """passes without the feature: it asserts on the restatement"""
    sc, r = scene("bad_voted"), ref("bad_voted")
    nm = sc["names"]  # the bad one has 8 votes, `good` 3, `other` 1
    assert (r.n_k1, r.local_kfs, r.ref_kf) == (2, [nm["good"], nm["other"]], nm["good"])
    k = scene("tie")["names"]["k"]
    assert ref("tie").ref_kf == k[1] and ref("tie").local_kfs == k
    assert ref("tie_ranked").ref_kf == k[3] and ref("tie_ranked").local_kfs == [k[2], k[3], k[0], k[1]]
    assert ref("tie").n_local == ref("tie_ranked").n_local == 9 and ref("tie").local_points != ref("tie_ranked").local_points
    sc, r = scene("all_voted_bad"), ref("all_voted_bad")  # not KEPT: somebody voted; the list is empty
    assert (r.status, r.n_k1, r.local_kfs, r.ref_kf, r.n_local, r.n_extra) == (lr.OK, 0, [], -1, 0, 2)
    assert (r.frame_mp[:2] == [0, 1]).all()
    sc, r = scene("no_votes"), ref("no_votes")
    nm = sc["names"]
    assert (r.status, r.local_kfs, r.ref_kf, r.n_k1) == (lr.KEPT, nm["prev"], -1, 0)
    # the previous list's order: b's eleven points, then nothing new from a (six shared, one bad)
    assert r.n_local == 11 and r.local_points == [int(p) for p in sc["mirror"]["slots"][nm["prev"][0]]]
    assert r.n_nulled == 1 and (r.frame_mp[nm["kp_bad"]] == -1).all() and r.n_extra == 2  # `lone` and the temporal point


# ---- CPU: points and extras -------------------------------------------------------------

def test_points_first_occurrence_extras_and_last_seen():
    """passes without the feature: it asserts on the restatement"""
    sc, r = scene("rich"), ref("rich")
    nm, M, J = sc["names"], sc["mirror"], sc["job"]
    assert r.status == lr.OK and r.local_kfs == [nm["a"], nm["b"], nm["c"]] and r.ref_kf == nm["b"]
    # seen from three keyframes: the position is a's slot (after a's seven own), not b's slot 0
    assert r.local_points.index(nm["seen3"]) == 7 and r.local_points.count(nm["seen3"]) == 1
    assert len(set(r.local_points)) == r.n_local and -1 not in r.local_points
    assert not set(nm["dead"]) & set(r.local_points) and all(M["pt_flags"][p] & lr.VALID for p in r.local_points)
    # the held bad point is nulled; extras in keypoint order, once each, after the local points
    assert r.n_nulled == 1 and (r.frame_mp[nm["kp_bad"]] == -1).all()
    assert r.n_extra == 5 and not set(nm["extra"]) & set(r.local_points)
    a, b = nm["kp_twice"]
    assert r.frame_mp[a] == r.frame_mp[b] >= r.n_local
    a, b = nm["kp_vo2"]
    assert r.frame_mp[a] == r.frame_mp[b] >= r.n_local and r.table["flags"][r.frame_mp[a]] == lr.VALID
    t = nm["vo"][1]
    assert r.table["desc"][r.frame_mp[a]].tobytes() == J["src_desc"][t].tobytes()
    assert r.table["pos"][r.frame_mp[a]].tobytes() == J["src_pos"][t].tobytes() and not r.table["normal"][r.frame_mp[a]].any()
    held_extra = [int(v) for v in r.frame_mp if v >= r.n_local]
    assert sorted(set(held_extra)) == list(range(r.n_local, r.n_local + 5))
    assert [held_extra.index(v) for v in sorted(set(held_extra))] == sorted(held_extra.index(v) for v in set(held_extra))
    # LAST_SEEN on exactly the culled points (a point culled at one keypoint and held at another is in row 1)
    flagged = [r.local_points[i] for i in np.nonzero(r.table["flags"][:r.n_local] & lr.LAST_SEEN)[0]]
    assert sorted(flagged) == sorted(nm["culled"]) and len(flagged) == 7
    assert (r.table["flags"][r.n_local:] & lr.LAST_SEEN == 0).all()
    i = r.local_points.index(nm["held"][0])
    assert r.table["flags"][i] == lr.VALID | lr.HAS_OBS and r.table["desc"][i].tobytes() == M["desc"][nm["held"][0]].tobytes()


def test_bad_ids_and_capacity_in_the_restatement():
    """passes without the feature: it asserts on the restatement"""
    for j in bad_jobs():
        assert lr.update_local_map(scene("rich")["mirror"], j, S, P, KS).status == lr.BAD_JOB
    sc = scene("rich")
    r = lr.update_local_map(sc["mirror"], sc["job"], S, 90, KS)
    assert (r.status, r.n_local, r.n_extra, r.points_n) == (lr.CAPACITY, 87, 5, 92)
    r = lr.update_local_map(sc["mirror"], sc["job"], S, P, 2)
    assert (r.status, r.n_local_kfs, r.n_local, r.points_n) == (lr.CAPACITY, 3, 0, P + 1)
    r = lr.update_local_map(sc["mirror"], dict(sc["job"], n_kp=S + 1), S, P, KS)
    assert (r.status, r.n_local_kfs, r.points_n) == (lr.CAPACITY, 0, P + 1)


# ---- CPU: child lists longer than the walk's staged look ----------------------------------------

LONG_BAD = [("c", 50), ("c", 89), ("b", 21), ("a", 20), ("c", 21)]  # past the staged 21, after the found one, at the edges


def test_long_child_lists_in_the_restatement():
    """passes without the feature: it asserts on the restatement"""
    sc, r = scene("long_children"), ref("long_children")
    nm = sc["names"]
    assert nm["sizes"] == [21, 22, 90] and r.status == lr.OK and r.n_k1 == 3
    assert r.local_kfs == nm["k1"] + nm["added"] and nm["never"] not in r.local_kfs
    M = sc["mirror"]
    for member, at in zip(nm["k1"], (20, 21, 87)):  # the added child's index, and nothing addable before it
        ch = M["children"][member]
        assert ch[at] in nm["added"] and all(M["kf_bad"][x] or x in r.local_kfs[:r.local_kfs.index(ch[at])] for x in ch[:at])
    for bc in LONG_BAD:
        b = ls.long_children(bad_child=bc)
        assert lr.update_local_map(b["mirror"], b["job"], S, P, KS).status == lr.BAD_JOB, bc


# ---- CPU: fed into track_ref ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chain_first():
    return ts.initial_batch([dict(groups=[dict(n=60), dict(n=10, shift_px=6.0)])], seed=62)


def chain_map(first, rows):
    """The chained frame's map as a mirror: the last frame's good slots are the points, all in one keyframe in
    slot order and observed from it, so the local map is track_scene.chain_local's without its NULL slots.
    Returns (mirror, job, slot of every point)."""
    J = first["jobs"][0]
    hand = ts.chain_local(first, 0, rows)["jobs"][0]["table"]
    slot = np.nonzero(J["table"]["flags"] & ts.VALID)[0]
    src = np.full(len(J["table"]["flags"]), -1, np.int32)
    src[slot] = np.arange(len(slot))
    n = len(slot)
    mirror = {"kf_bad": np.zeros(1, np.uint8), "slots": [np.arange(n, dtype=np.int32)],
              "covis": np.full((1, 10), -1, np.int32), "children": [[]], "parent": np.array([-1], np.int32),
              "kf_by_rank": None, "pt_flags": np.asarray(J["table"]["flags"][slot], np.int32), "obs": [[0]] * n,
              "pos": hand["pos"][slot], "normal": hand["normal"][slot], "desc": hand["desc"][slot],
              "min_dist": hand["min_dist"][slot], "max_dist": hand["max_dist"][slot]}
    job = {"n_kp": len(rows[0]), "rows": np.asarray(rows, np.int32), "src_pt_id": src, "src_pos": J["table"]["pos"],
           "src_desc": J["table"]["desc"], "prev_kfs": []}
    return mirror, job, slot


def as_local_batch(first, r, th=3.0):
    """localmap_ref's output as a track_scene.local_batch of one frame"""
    job = {"frame": 0, "Tcw": None, "frame_mp": r.frame_mp.copy(), "n_local": r.n_local, "th": float(th),
           "stereo": int(first["stereo"]), "only_tracking": 0, "recently_relocalised": 0, "table": r.table, "groups": {}}
    return {"stereo": first["stereo"], "frames": [first["frames"][0]], "jobs": [job]}


@functools.lru_cache(maxsize=None)
def chain_cpu():
    first = chain_first()
    r1 = tr.track_initial(first, 0)
    mirror, job, slot = chain_map(first, r1.rows)
    lm = lr.update_local_map(mirror, job, ts.N_KP, len(slot) + 8, 4)
    return r1, slot, lm, tr.track_local(as_local_batch(first, lm), 0, Tcw=r1.Tcw)


def test_table_of_the_restatement_tracks_like_the_hand_built_one():
    """passes without the feature: it asserts on the restatement.  The hand-built table keeps the last frame's
    NULL slots as invalid entries and UpdateLocalPoints never lists them, so indices map through `slot`."""
    r1, slot, lm, got = chain_cpu()
    assert lm.status == lr.OK and lm.n_local == len(slot) and lm.n_extra == 0 and lm.local_points == list(range(len(slot)))
    hand = ts.chain_local(chain_first(), 0, r1.rows)
    want = tr.track_local(hand, 0, Tcw=r1.Tcw)
    assert np.array_equal(slot[lm.frame_mp[lm.frame_mp >= 0]], hand["jobs"][0]["frame_mp"][lm.frame_mp >= 0])
    assert np.array_equal(lm.frame_mp >= 0, hand["jobs"][0]["frame_mp"] >= 0)
    kp, pt = hand["jobs"][0]["groups"]["culled"]
    assert np.array_equal(slot[np.nonzero(lm.table["flags"] & lr.LAST_SEEN)[0]], np.sort(pt)) and len(pt) >= 3
    assert (got.status, got.n_to_match, got.nsearch, got.n_inliers) == (want.status, want.n_to_match, want.nsearch,
                                                                        want.n_inliers) and got.status == tr.OK
    assert np.asarray(got.Tcw, np.float32).tobytes() == np.asarray(want.Tcw, np.float32).tobytes()
    for k in range(2):
        assert np.array_equal(got.rows[k] >= 0, want.rows[k] >= 0)
        assert np.array_equal(slot[got.rows[k][got.rows[k] >= 0]], want.rows[k][want.rows[k] >= 0])
    assert np.array_equal(got.rows[2], want.rows[2]) and np.array_equal(got.point_flags, want.point_flags[slot])


# ---- without a GPU: the entry point's host side ------------------------------------------------

def test_library_has_the_local_map_entry_points():
    """fails without the feature: the library has no orbgpu_update_local_map_* symbols"""
    import orbgpu
    L = orbgpu.lib()
    for name in ("orbgpu_update_local_map_workspace_bytes", "orbgpu_update_local_map_batch_device"):
        assert hasattr(L, name), name


def test_argument_errors_come_before_the_device():
    import track
    L = track._lib()
    p = ctypes.c_void_p(256)  # never dereferenced

    def mirror(**kw):
        m = track.MapMirrorStruct()
        m.n_kf, m.n_pt, m.n_slots_total, m.n_children_total, m.n_obs_total = 2, 3, 4, 1, 3
        for name, _ in track.MapMirrorStruct._fields_[6:]:
            setattr(m, name, 256)
        for k, v in kw.items():
            setattr(m, k, v)
        return ctypes.byref(m)

    def call(n=1, jobs=p, m=None, stride=8, ps=8, ks=8, ws=p, res=p, kfs=p, pts=p):
        return L.orbgpu_update_local_map_batch_device(n, jobs, m if m is not None else mirror(), stride, ps, ks, ws, res,
                                                      kfs, pts, None)

    for kw in (dict(n=-1), dict(stride=0), dict(ps=0), dict(ks=0), dict(jobs=None), dict(ws=None), dict(res=None),
               dict(kfs=None), dict(pts=None), dict(n=1 << 20, stride=1 << 12), dict(n=1 << 20, ps=1 << 12),
               dict(n=1 << 20, ks=1 << 12), dict(m=mirror(n_kf=-1)), dict(m=mirror(n_pt=-1)), dict(m=mirror(n_obs_total=-1)),
               dict(m=mirror(kf_bad=None)), dict(m=mirror(slots=None)), dict(m=mirror(children=None)),
               dict(m=mirror(parent=None)), dict(m=mirror(pt_flags=None)), dict(m=mirror(obs=None)),
               dict(m=mirror(desc=None)), dict(m=mirror(max_dist=None))):
        assert call(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    assert L.orbgpu_update_local_map_batch_device(1, p, None, 8, 8, 8, p, p, p, p, None) == -1  # no mirror
    assert L.orbgpu_update_local_map_batch_device(0, None, None, 8, 8, 8, None, None, None, None, None) == 0
    assert L.orbgpu_update_local_map_workspace_bytes(3, 300, 500, 96, 20, 1000) > 0


@pytest.fixture(scope="module")
def localmap_args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("localmap_args") / "localmap_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "localmap_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_point_is_clean_under_the_sanitizers(localmap_args_main):
    """argument checks and the carving of the opaque block from a null base, compiled for the host with
    -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(localmap_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layouts_equal_the_header(localmap_args_main):
    import track
    r = subprocess.run([str(localmap_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = dict(re.findall(r"(\S+) (\d+)", r.stdout))
    M, J, R = track.MapMirrorStruct, track.UpdateLocalMapJob, track.UpdateLocalMapResult
    want = {"orbgpu_map_mirror": ctypes.sizeof(M), "orbgpu_update_local_map_job": ctypes.sizeof(J),
            "orbgpu_update_local_map_result": ctypes.sizeof(R), "mirror.kf_bad": M.kf_bad.offset,
            "mirror.kf_by_rank": M.kf_by_rank.offset, "mirror.obs": M.obs.offset, "mirror.max_dist": M.max_dist.offset,
            "job.rows": J.rows.offset, "job.prev_kfs": J.prev_kfs.offset, "job.out_desc": J.out_desc.offset,
            "job.local_job": J.local_job.offset, "result.ref_kf": R.ref_kf.offset, "result.n_extra": R.n_extra.offset}
    assert {k: int(v) for k, v in got.items()} == want


# ---- GPU -----------------------------------------------------------------------------------

def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def lm_step(stride):
    """a TrackStep for update_local_map alone: the call reads no frame"""
    import track
    return track.TrackStep(SimpleNamespace(device="cuda", stride=stride, n_f=1))


def upload(mirror):
    import track
    return track.MapMirror(**mirror)


def run_lm(torch, mirror, jobs, stride=S, point_stride=P, kf_stride=KS, step=None, d_mirror=None):
    """The call for `jobs` on one mirror with every output buffer filled with GUARD bytes first.  Returns a
    namespace: res (the result structs), raw (their bytes per job), kfs, pts, mp, tab (numpy), prepared (call 2's
    jobs), step."""
    step = step or lm_step(stride)
    if not hasattr(step, "d_table"):
        step.prepare_local_map([dict(frame=0, Tcw=None, th=1.0) for _ in jobs], point_stride)
    import track
    tables = [track.PointTable(np.zeros(len(j["src_pt_id"]), np.int32), j["src_pos"], desc=j["src_desc"]) for j in jobs]
    step.update_local_map([dict(n_kp=j["n_kp"], rows=j["rows"], src_pt_id=j["src_pt_id"], table=t, prev_kfs=j["prev_kfs"])
                           for j, t in zip(jobs, tables)], d_mirror or upload(mirror), kf_stride=kf_stride, launch=False)
    for t in list(step.d_table.values()) + [step.d_frame_mp, step.d_local_kfs, step.d_local_points, step.d_lm_results]:
        t.view(torch.uint8).fill_(GUARD)
    step.lm_ws.fill_(GUARD)  # the workspace need not be zeroed
    step.run_update_local_map()
    torch.cuda.synchronize()
    raw = bytes(step.d_lm_results.cpu().numpy())
    sz = 32
    return SimpleNamespace(res=step.update_results(), raw=[raw[i * sz:(i + 1) * sz] for i in range(len(jobs))],
                           kfs=step.local_kfs(), pts=step.local_points(), mp=step.prepared_frame_mp(),
                           tab=step.prepared_tables(), prepared=step.prepared_jobs(), step=step)


def guard(a):
    return (np.ascontiguousarray(a).view(np.uint8) == GUARD).all()


def assert_job(g, k, r, where, stride=S, point_stride=P, kf_stride=KS):
    """job k of the run g against the reference r: every int, every table byte, and the guard bytes past them"""
    R = g.res[k]
    assert (R.status, R.n_k1, R.n_local_kfs, R.ref_kf, R.n_nulled, R.n_local, R.n_extra, R.pad) == \
        (r.status, r.n_k1, r.n_local_kfs, r.ref_kf, r.n_nulled, r.n_local, r.n_extra, 0), where
    L = g.prepared[k]
    if r.status == lr.BAD_JOB:  # nothing but the result, and frame = -1 in the prepared job
        assert guard(g.kfs[k]) and guard(g.pts[k]) and guard(g.mp[k]) and all(guard(t[k]) for t in g.tab.values()), where
        assert (L.frame, L.n_local, L.points.n, L.frame_mp, L.points.flags) == (-1, 0, 0, None, None), where
        return
    n_kf, n_lp, n_tab = min(r.n_local_kfs, kf_stride), min(r.n_local, point_stride), min(r.points_n, point_stride)
    assert g.kfs[k][:n_kf].tolist() == r.local_kfs[:n_kf] and guard(g.kfs[k][n_kf:]), where
    assert g.pts[k][:n_lp].tolist() == r.local_points[:n_lp] and guard(g.pts[k][n_lp:]), where
    n_kp = len(r.frame_mp) if r.frame_mp is not None and r.table is not None else 0
    assert np.array_equal(g.mp[k][:n_kp], r.frame_mp[:n_kp]) and (g.mp[k][n_kp:] == -1).all(), where
    if r.table is None:
        n_tab = 0
    for name, t in g.tab.items():
        if n_tab:
            assert t[k][:n_tab].tobytes() == np.ascontiguousarray(r.table[name][:n_tab]).tobytes(), (where, name)
        assert guard(t[k][n_tab:]), (where, name)
    step = g.step
    assert (L.frame, L.n_local, L.points.n) == (0, r.n_local_job, r.points_n), where
    assert L.frame_mp == step.d_frame_mp[k].data_ptr() and L.points.flags == step.d_table["flags"][k].data_ptr(), where
    for name in ("pos", "normal", "desc", "min_dist", "max_dist"):
        assert getattr(L.points, name) == step.d_table[name][k].data_ptr(), (where, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ls.SCENES))
def test_gpu_named_scenes_equal_the_restatement(name):
    torch = _gpu()
    sc = scene(name)
    g = run_lm(torch, sc["mirror"], [sc["job"]])
    assert_job(g, 0, ref(name), name)


SIZES = [(0, 0), (1, 1), (63, 64), (64, 65), (65, 300), (255, 0), (256, 1), (257, 64), (700, 300), (0, 65), (0, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_local,n_held", SIZES)
def test_gpu_edge_sizes(n_local, n_held):
    """local point counts around the wave, the 256-slot tile and above it, over keyframes whose slot counts are no
    multiples of 64; 0, 1, 64, 65 and 300 held keypoints; 300 extras are more than one 256-entry stripe of the extras' ranking"""
    torch = _gpu()
    sc = ls.sized(n_local, n_held)
    r = lr.update_local_map(sc["mirror"], sc["job"], S, P, KS)
    assert r.n_local == n_local and sc["job"]["n_kp"] == n_held + 2 and r.n_extra == max(n_held - n_local, 0)
    assert r.status == (lr.OK if n_local and n_held else lr.KEPT)
    assert all(len(s) % 64 for s in sc["mirror"]["slots"] if len(s)) and (n_local < 700 or max(map(len, sc["mirror"]["slots"])) > 512)
    assert_job(run_lm(torch, sc["mirror"], [sc["job"]]), 0, r, (n_local, n_held))


@pytest.mark.gpu
@pytest.mark.parametrize("bad_child", LONG_BAD)
def test_gpu_long_child_list_with_an_id_outside_the_map(bad_child):
    """every child of a visited keyframe is range-checked, the ones read from memory past the staged 21 too"""
    torch = _gpu()
    sc = ls.long_children(bad_child=bad_child)
    r = lr.update_local_map(sc["mirror"], sc["job"], S, P, KS)
    assert r.status == lr.BAD_JOB
    assert_job(run_lm(torch, sc["mirror"], [sc["job"]]), 0, r, bad_child)


def shared_jobs():
    """three jobs on the `rich` mirror: the scene's; nobody holds anything but a temporal point, so the previous
    list stands; every other keypoint"""
    sc = scene("rich")
    J, nm = sc["job"], sc["names"]
    none = np.full_like(J["rows"], -1)
    none[:, nm["kp_vo2"]] = J["rows"][:, nm["kp_vo2"]]
    kept = dict(J, rows=none, prev_kfs=[nm["c"], nm["a"]])
    half = dict(J, rows=np.ascontiguousarray(J["rows"][:, ::2]), n_kp=(J["n_kp"] + 1) // 2)
    return sc["mirror"], [J, kept, half]


def bad_jobs():
    """the `rich` job with one id outside the mirror each"""
    sc = scene("rich")
    J, M = sc["job"], sc["mirror"]
    n_pt, t = len(M["pt_flags"]), int(J["rows"][1][0])
    out = []
    for v in (n_pt, -2):
        src = J["src_pt_id"].copy()
        src[t] = v
        out.append(dict(J, src_pt_id=src))
    rows = J["rows"].copy()
    rows[0][3] = len(J["src_pt_id"])  # a row entry beyond call 1's table
    out.append(dict(J, rows=rows))
    out.append(dict(J, rows=np.full_like(J["rows"], -1), prev_kfs=[0, len(M["kf_bad"])]))  # the previous list, when read
    return out


def bad_mirrors():
    """the `rich` mirror with one id out of range where the job reads it: a local keyframe's slot, a held point's
    observation, a visited keyframe's covisible, child and parent"""
    M = scene("rich")["mirror"]
    a, n_kf, n_pt = scene("rich")["names"]["a"], len(M["kf_bad"]), len(M["pt_flags"])
    held = int(scene("rich")["job"]["src_pt_id"][scene("rich")["job"]["rows"][1][0]])
    out = []
    slots = [s.copy() for s in M["slots"]]
    slots[a][1] = n_pt
    out.append(dict(M, slots=slots))
    slots = [s.copy() for s in M["slots"]]
    slots[a][0] = -2
    out.append(dict(M, slots=slots))
    obs = [list(o) for o in M["obs"]]
    obs[held] = obs[held] + [n_kf]
    out.append(dict(M, obs=obs))
    cov = M["covis"].copy()
    cov[a, 9] = n_kf
    out.append(dict(M, covis=cov))
    ch = [list(c) for c in M["children"]]
    ch[a] = [-1]
    out.append(dict(M, children=ch))
    par = M["parent"].copy()
    par[a] = -2
    out.append(dict(M, parent=par))
    out.append(dict(M, kf_by_rank=np.array([0, 1, 2, 3, n_kf], np.int32)))
    return out


@pytest.mark.gpu
def test_gpu_results_do_not_depend_on_the_batch_the_position_or_the_run():
    """three jobs on one shared mirror: the same bytes alone, first, last and in a second run"""
    torch = _gpu()
    mirror, jobs = shared_jobs()
    d_mirror = upload(mirror)
    refs = [lr.update_local_map(mirror, j, S, P, KS) for j in jobs]
    assert [r.status for r in refs] == [lr.OK, lr.KEPT, lr.OK] and refs[2].points_n != refs[0].points_n

    def snap(g, at):
        return (g.raw[at], g.kfs[at].tobytes(), g.pts[at].tobytes(), g.mp[at].tobytes(),
                tuple(t[at].tobytes() for t in g.tab.values()))

    whole = run_lm(torch, mirror, jobs, d_mirror=d_mirror)
    for k in range(3):
        assert_job(whole, k, refs[k], k)
    again = run_lm(torch, mirror, jobs, d_mirror=d_mirror)
    whole.step.run_update_local_map()  # and on the workspace the first run left behind
    torch.cuda.synchronize()
    rerun = SimpleNamespace(raw=[bytes(whole.step.d_lm_results.cpu().numpy())[32 * i:32 * i + 32] for i in range(3)],
                            kfs=whole.step.local_kfs(), pts=whole.step.local_points(), mp=whole.step.prepared_frame_mp(),
                            tab=whole.step.prepared_tables())
    for q in range(3):
        others = [k for k in range(3) if k != q]
        alone = run_lm(torch, mirror, [jobs[q]], d_mirror=d_mirror)
        head = run_lm(torch, mirror, [jobs[k] for k in [q] + others], d_mirror=d_mirror)
        tail = run_lm(torch, mirror, [jobs[k] for k in others + [q]], d_mirror=d_mirror)
        for got, at in ((alone, 0), (head, 0), (tail, 2), (again, q), (rerun, q)):
            assert snap(got, at) == snap(whole, q), (q, at)


@pytest.mark.gpu
def test_gpu_capacity_and_bad_jobs_end_alone():
    """CAPACITY through the points, the keyframes and the keypoints, and BAD_JOB through every id the job reads:
    each equals the restatement with the guard bytes intact, and so do its neighbours in the batch.  The bad ids
    are ordinary input: every one is range-checked before it is used."""
    torch = _gpu()
    mirror, jobs = shared_jobs()
    d_mirror = upload(mirror)
    for dims in (dict(point_stride=90), dict(point_stride=87), dict(point_stride=92), dict(kf_stride=2), dict(stride=40)):
        d = dict(dict(stride=S, point_stride=P, kf_stride=KS), **dims)
        refs = [lr.update_local_map(mirror, j, d["stride"], d["point_stride"], d["kf_stride"]) for j in jobs]
        g = run_lm(torch, mirror, jobs, d_mirror=d_mirror, **d)
        for k in range(3):
            assert_job(g, k, refs[k], (dims, k), **d)
        want = {"point_stride": {90: [lr.CAPACITY, lr.KEPT, lr.OK], 87: [lr.CAPACITY, lr.KEPT, lr.CAPACITY],
                                 92: [lr.OK, lr.KEPT, lr.OK]}.get(d["point_stride"]),
                "kf_stride": [lr.CAPACITY, lr.KEPT, lr.CAPACITY], "stride": [lr.CAPACITY, lr.CAPACITY, lr.OK]}[list(dims)[0]]
        assert [r.status for r in refs] == want, dims
    clean = [lr.update_local_map(mirror, j, S, P, KS) for j in jobs]
    for bad in bad_jobs():
        batch = [jobs[0], bad, jobs[2]]
        g = run_lm(torch, mirror, batch, d_mirror=d_mirror)
        r = lr.update_local_map(mirror, bad, S, P, KS)
        assert r.status == lr.BAD_JOB
        for k, want in enumerate((clean[0], r, clean[2])):
            assert_job(g, k, want, k)
    spared = 0
    for bm in bad_mirrors():
        refs = [lr.update_local_map(bm, j, S, P, KS) for j in jobs]
        assert refs[0].status == lr.BAD_JOB
        spared += refs[1].status == lr.KEPT  # a job that never reads the id is not touched by it
        g = run_lm(torch, bm, jobs)
        for k in range(3):
            assert_job(g, k, refs[k], k)
    assert spared >= 3


@pytest.mark.gpu
def test_gpu_chain_is_three_calls_on_one_stream():
    """initial -> update_local_map -> local_map enqueued on one stream with no host call between them.  Call 2's
    result, rows and point flags equal track_ref fed by localmap_ref (the pose within tests/test_track.py's
    bound, by its helper), and equal byte for byte the existing path: TrackStep.local_map with the table built
    on the host."""
    torch = _gpu()
    import test_track as tt
    import track
    first = chain_first()
    step = tt.gpu_step(first)
    J = dict(first["jobs"][0])
    J["table"] = track.PointTable(**J["table"])
    step.initial([J])
    torch.cuda.synchronize()
    rows1 = step.initial_rows()[0].copy()
    mirror, job, slot = chain_map(first, rows1)
    lm = lr.update_local_map(mirror, job, ts.N_KP, len(slot) + 8, 4)
    step.prepare_local_map([dict(frame=0, Tcw=step.initial_pose_ptr(0), th=3.0, stereo=int(first["stereo"]))], len(slot) + 8)
    step.update_local_map([dict(n_kp=ts.N_KP, src_pt_id=job["src_pt_id"], table=J["table"], prev_kfs=[])],
                          upload(mirror), kf_stride=4, launch=False)
    for t in (step.d_initial_rows, step.d_initial_results, step.d_frame_mp, step.d_local_results, step.d_local_rows):
        t.view(torch.uint8).fill_(GUARD)  # nothing of the first run is left for the chain to lean on
    stream = torch.cuda.Stream()
    step.run_initial(stream)
    step.run_update_local_map(stream)
    step.run_local_map(stream)
    stream.synchronize()
    assert np.array_equal(step.initial_rows()[0], rows1)
    g = SimpleNamespace(res=step.update_results(), kfs=step.local_kfs(), pts=step.local_points(),
                        mp=step.prepared_frame_mp(), tab=step.prepared_tables(), prepared=step.prepared_jobs(), step=step)
    R = g.res[0]
    assert (R.status, R.n_local, R.n_extra, R.n_local_kfs, R.ref_kf) == (lr.OK, lm.n_local, 0, 1, 0)
    assert g.pts[0][:lm.n_local].tolist() == lm.local_points and np.array_equal(g.mp[0], lm.frame_mp)
    for name, t in g.tab.items():
        assert t[0][:lm.points_n].tobytes() == np.ascontiguousarray(lm.table[name]).tobytes(), name
    pose = tt.T4(step.initial_results()[0].Tcw)
    second = as_local_batch(first, lm)
    want = tr.track_local(second, 0, Tcw=pose)
    assert want.status == tr.OK and tr.decisive(want) is None
    res, rows, pf = step.local_results(), step.local_rows(), step.point_flags()
    tt.assert_local(res[0], rows[0], pf[0], want, "chain, call 2")
    ptr = step.initial_pose_ptr(0)
    host = tt.run_local(torch, second, edit=lambda k, J: J.update(Tcw=ptr), point_stride=len(slot) + 8)
    assert bytes(step.d_local_results.cpu().numpy()) == b"".join(host[0])
    assert np.array_equal(rows, host[1]) and np.array_equal(pf, host[3])


@pytest.mark.gpu
def test_gpu_call_2_reports_capacity_and_bad_job_for_exactly_those_jobs():
    """call 2 on the prepared jobs, nothing uploaded in between: ORBGPU_TRACK_CAPACITY for the job whose points
    exceed point_stride and the one whose keyframes exceed kf_stride, ORBGPU_TRACK_BAD_JOB for the one with an id
    outside the mirror, neither for the fourth"""
    torch = _gpu()
    import test_track as tt
    mirror, jobs = shared_jobs()
    batch = ts.local_batch([dict(groups=[], n_local=8)] * 4, seed=71)
    step = tt.gpu_step(batch)
    many = dict(jobs[0], prev_kfs=[])
    few = jobs[1]  # the kept job: two keyframes, few points
    five = dict(jobs[1], prev_kfs=[0, 1, 2, 3, 4])
    batch_jobs = [many, bad_jobs()[0], few, five]
    refs = [lr.update_local_map(mirror, j, ts.N_KP, 60, 4) for j in batch_jobs]
    assert [r.status for r in refs] == [lr.CAPACITY, lr.BAD_JOB, lr.KEPT, lr.CAPACITY]
    assert refs[0].points_n == 92 and refs[3].points_n == 61
    pose = np.eye(4, dtype=np.float32)
    step.prepare_local_map([dict(frame=k, Tcw=pose, th=1.0) for k in range(4)], 60)
    g = run_lm(torch, mirror, batch_jobs, stride=ts.N_KP, point_stride=60, kf_stride=4, step=step)
    for k in range(4):
        R = g.res[k]
        assert (R.status, R.n_local, R.n_extra, R.n_local_kfs) == (refs[k].status, refs[k].n_local, refs[k].n_extra,
                                                                   refs[k].n_local_kfs), k
    step.run_local_map()
    torch.cuda.synchronize()
    got = [r.status for r in step.local_results()]
    assert got[0] == tr.CAPACITY and got[1] == tr.BAD_JOB and got[3] == tr.CAPACITY
    assert got[2] in (tr.OK, tr.LOST)
