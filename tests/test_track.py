"""Tracking's per-frame chain on the device (src/Tracking.cpp:977-1264,
:1496-1562): orbgpu_track_initial_batch_device,
orbgpu_track_local_map_batch_device and orbgpu_update_last_frame_batch_device
(csrc/track.hip) against tests/track_ref.py on tests/track_scene.py scenes
(batches of 3 frames, 300 keypoints, a few hundred table entries).

CPU (these pass without the library's new entry points, by construction: they
assert on the reference).  Call 1 takes every path -- a first search >= 20; a
first search < 20 with the 2*th retry >= 20 from an all-NULL row; both < 20; a
cull that leaves nmatchesMap >= 10; one that leaves < 10 through points without
observations (LOST, and OK with vo under only_tracking); only_tracking failing
on nmatches; monocular and stereo frames; a rotation cull with -2 entries;
reference mode below and above 15 BoW matches.  Call 2 likewise -- nToMatch ==
0; a held bad point nulled; a seen point not re-projected; a keypoint holding
a point without observations reassigned and one with observations kept;
stereo nulling outliers and non-stereo keeping them; 30 and 50 from both sides;
only_tracking counting; th 1, 3, 5; n_local == 0; a point culled by call 1, in
the local map and in the frustum, skipped.  Every scene is decisive
(track_ref.decisive).  UpdateLastFrame: the literal loop against the closed
form the kernel uses.  Argument errors come before the device, track.py's
structs have the header's layout, and the host side of the entry points runs
clean under the address and undefined-behaviour sanitizers as a program of its
own (tests/cpp/track_args_main.cpp).

GPU: every integer of every result and row equal to the reference; call 3's
bytes equal; gathers of 63 / 64 / 65; call 2 made from call 1's rows and reading its pose
in place, the culled points neither counted nor matched;
independence of the batch, the position and the run; an over-capacity frame,
a bad job and a NaN pose end alone.

Tolerance.  The searches are integer-exact and the gathers copy floats, so each
optimisation starts from the reference's bits (call 2's reference is fed the
GPU's input pose bits): each Tcw is held to tests/test_poseopt.py's bound, 2
float32 ulp at scale max(1, max |Tcw|).
"""
import ctypes
import functools
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import track_ref as tr
import track_scene as ts

ROOT = Path(__file__).resolve().parent.parent
ULP = 2.0 ** -23


def G(n, **k):
    return dict(n=n, **k)


def H(n, **k):
    return dict(n=n, held=True, **k)


INITIAL = {
    # first search >= 20 with a cull; the retry; both searches < 20
    "mono": dict(seed=31, specs=[dict(groups=[G(60), G(10, shift_px=6.0)]),
                                 dict(groups=[G(50), G(8, at_init=True)], init_shift_px=21.0, octaves=(0, 0)),
                                 dict(groups=[G(9)])]),
    # nmatchesMap < 10 through points without observations: LOST, OK + vo; only_tracking failing on nmatches
    "mono2": dict(seed=32, specs=[dict(groups=[G(30, obs=False), G(5)]),
                                  dict(groups=[G(30, obs=False), G(5)], only_tracking=1),
                                  dict(groups=[G(16), G(9, shift_px=6.0)], only_tracking=1)]),
    # bMono false with u_right, th 7: a fourth rotation bin culled; the retry; the camera moving backwards
    "stereo": dict(seed=33, stereo=True,
                   specs=[dict(groups=[G(40), G(12, bin=5), G(12, bin=10), G(4, bin=15)], forward=0.5),
                          dict(groups=[G(50), G(8, at_init=True)], init_shift_px=10.5, octaves=(0, 0)),
                          dict(groups=[G(45), G(10, shift_px=6.0)], forward=-0.5)]),
    "reference": dict(seed=34, specs=[dict(mode=1, groups=[G(9)]),
                                      dict(mode=1, groups=[G(40), G(8, shift_px=6.0)]),
                                      dict(mode=1, groups=[G(30, obs=False), G(4)])]),
    "edges": dict(seed=35, kp_noise=0.05, specs=[dict(groups=[G(63 + q)]) for q in range(3)]),
}
RICH = [H(30, name="held"), H(5, bad=True, name="bad"), H(10, where="extra", obs=False, name="vo"), G(25, name="new"),
        G(5, view="wide", name="wide"), G(5, view="cos", name="cos"), G(6, onto="noobs", name="reassign"),
        G(6, onto="obs", name="kept"), H(6, shift_px=6.0, name="out")]
PAIR = [H(20, name="held"), G(20, name="new")]
HALF = [H(20, name="held"), H(20, where="extra", obs=False, name="vo")]
LOCAL = {
    "a": dict(seed=41, specs=[dict(groups=RICH, n_local=200, n_extra=40, th=1, recently_relocalised=1),
                              dict(groups=PAIR, n_local=150, n_extra=10, th=3, pose_shift_px=4.0),
                              dict(groups=PAIR, n_local=150, n_extra=10, th=5, pose_shift_px=8.0,
                                   recently_relocalised=1)]),
    "b": dict(seed=42, stereo=True,
              specs=[dict(groups=[H(40, name="held"), H(8, shift_px=6.0, name="out"), G(20, name="new")], n_local=150,
                          n_extra=10),
                     dict(groups=[H(12, name="held"), G(8, name="new")], n_local=100, n_extra=10),
                     dict(groups=HALF, n_local=100, n_extra=30, only_tracking=1)]),
    "c": dict(seed=43, specs=[dict(groups=[H(50, name="held")], n_local=50, n_extra=0),
                              dict(groups=[H(40, where="extra", name="held")], n_local=0, n_extra=40),
                              dict(groups=HALF, n_local=100, n_extra=30)]),
    "edges": dict(seed=44, kp_noise=0.05,
                  specs=[dict(groups=[H(63 + q, where="extra")], n_local=0, n_extra=70) for q in range(3)]),
}


@functools.lru_cache(maxsize=None)
def ibatch(name):
    return ts.initial_batch(**INITIAL[name])


@functools.lru_cache(maxsize=None)
def iref(name):
    """the reference of every frame of a call-1 batch, computed once per session"""
    return tuple(tr.track_initial(ibatch(name), j) for j in range(3))


@functools.lru_cache(maxsize=None)
def lbatch(name):
    return ts.local_batch(**LOCAL[name])


@functools.lru_cache(maxsize=None)
def lref(name):
    return tuple(tr.track_local(lbatch(name), j) for j in range(3))


# ---- CPU: call 1 ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(INITIAL))
def test_initial_reference_is_decisive(name):
    """passes without the new entry points: it asserts on the reference"""
    for j, r in enumerate(iref(name)):
        assert tr.decisive(r) is None, (name, j)


def test_initial_reference_first_search_retry_and_both_short():
    """passes without the new entry points: it asserts on the reference"""
    first, retry, few = iref("mono")
    assert (first.status, first.searches) == (tr.OK, 1) and first.nsearch[0] >= 23 and first.nsearch[1] == -1
    assert (retry.status, retry.searches) == (tr.OK, 2) and retry.nsearch[0] <= 17 and retry.nsearch[1] >= 23
    # the projections lie between th and 2*th times the octave's scale factor from the keypoints
    b, J = ibatch("mono"), ibatch("mono")["jobs"][1]
    f = b["frames"][1]
    T = np.asarray(J["Tcw_init"], np.float64)
    src = np.array(sorted(k for k, s in J["pairs"].items() if retry.rows[1][k] == s))  # the pairs the cull kept
    assert len(src) >= 23
    Xc = f["Xw"][src] @ T[:3, :3].T + T[:3, 3]
    du = np.abs(ts.K[0] * Xc[:, 0] / Xc[:, 2] + ts.K[2] - f["kps"]["x"][src])
    dv = np.abs(ts.K[1] * Xc[:, 1] / Xc[:, 2] + ts.K[3] - f["kps"]["y"][src])
    r = J["th"] * ts.SF[f["kps"]["octave"][src]]
    assert (np.maximum(du, dv) > r).all() and (np.maximum(du, dv) < 2 * r).all()
    # the retry starts from an all-NULL row, although the first search left assignments behind
    held = retry.calls[0]["row"] >= 0  # they hold points with observations, which would hide them (ORBmatcher.cpp:1579)
    assert held.sum() == retry.nsearch[0] >= 3 and (J["table"]["flags"][retry.calls[0]["row"][held]] & tr.HAS_OBS).all()
    assert not retry.calls[1]["occupied"].any() and (retry.calls[1]["row"][held] >= 0).all()
    assert (few.status, few.searches) == (tr.FEW_MATCHES, 2) and max(few.nsearch) <= 17 and few.opt is None
    assert few.Tcw.tobytes() == np.asarray(ibatch("mono")["jobs"][2]["Tcw_init"], np.float32).tobytes()
    assert all((r >= 0).sum() == 0 for r in few.rows)


def test_initial_reference_culls_and_counts():
    """passes without the new entry points: it asserts on the reference"""
    first = iref("mono")[0]
    culled = (first.rows[0] >= 0).sum() - (first.rows[1] >= 0).sum()
    assert culled >= 3 and first.nmatches == first.nsearch[0] - culled and first.nmatches_map >= 13
    lost, vo, fail = iref("mono2")
    assert (lost.status, lost.vo) == (tr.LOST, 0) and lost.nmatches >= 23 and lost.nmatches_map <= 7
    assert (vo.status, vo.vo) == (tr.OK, 1) and vo.nmatches >= 23 and vo.nmatches_map <= 7
    assert fail.status == tr.LOST and fail.nsearch[0] >= 23 and fail.nmatches <= 17 and fail.nmatches_map >= 13
    assert fail.vo == 0


def test_initial_reference_stereo_and_the_rotation_cull():
    """passes without the new entry points: it asserts on the reference"""
    assert ibatch("mono")["frames"][0]["u_right"] is None and all(j["mono"] for j in ibatch("mono")["jobs"])
    b = ibatch("stereo")
    assert all((f["u_right"] > 0).all() for f in b["frames"]) and not any(j["mono"] for j in b["jobs"])
    assert [j["th"] for j in b["jobs"]] == [7.0] * 3
    rot, retry, back = iref("stereo")
    row = rot.calls[0]["row"]
    assert (row == -2).sum() == 4 and rot.nsearch[0] == (row >= 0).sum() and (rot.rows[0][row == -2] == -1).all()
    assert retry.searches == 2 and retry.nsearch[0] <= 17 and retry.nsearch[1] >= 23
    assert back.status == tr.OK and (back.rows[0] >= 0).sum() - (back.rows[1] >= 0).sum() >= 3


def test_initial_reference_mode():
    """passes without the new entry points: it asserts on the reference"""
    few, ok, lost = iref("reference")
    assert few.status == tr.FEW_MATCHES and few.nmatches <= 12 and few.opt is None and few.searches == 0
    assert ok.status == tr.OK and ok.searches == 0 and ok.nsearch == [-1, -1]
    assert (ok.rows[0] >= 0).sum() >= 18 and (ok.rows[0] >= 0).sum() - (ok.rows[1] >= 0).sum() >= 3
    assert np.array_equal(ok.rows[0], ibatch("reference")["jobs"][1]["bow_row"])  # the row itself is mvpMapPoints
    assert lost.status == tr.LOST and lost.nmatches_map <= 7


# ---- CPU: call 2 ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(LOCAL))
def test_local_reference_is_decisive(name):
    """passes without the new entry points: it asserts on the reference"""
    for j, r in enumerate(lref(name)):
        assert tr.decisive(r) is None, (name, j)


def test_local_reference_search_local_points():
    """passes without the new entry points: it asserts on the reference"""
    J, r = lbatch("a")["jobs"][0], lref("a")[0]
    g = J["groups"]
    kp, pt = g["bad"]
    assert (J["frame_mp"][kp] == pt).all() and (r.rows[0][kp] == -1).all() and not r.point_flags[pt].any()
    kp, pt = g["held"]  # seen: in the frustum, yet not projected again
    assert r.in_frustum[pt].all() and (r.point_flags[pt] == tr.PT_SEEN).all() and (r.rows[0][kp] == pt).all()
    for name in ("new", "wide"):
        kp, pt = g[name]
        assert (r.rows[0][kp] == pt).all() and (r.point_flags[pt] == tr.PT_IN_VIEW).all()
    kp, pt = g["cos"]  # viewCos < 0.5
    assert not r.in_frustum[pt].any() and (r.rows[0][kp] == -1).all() and not r.point_flags[pt].any()
    flags = J["table"]["flags"]
    kp, pt = g["reassign"]  # the keypoint held a point without observations
    assert (J["frame_mp"][kp] >= J["n_local"]).all() and not (flags[J["frame_mp"][kp]] & tr.HAS_OBS).any()
    assert (r.rows[0][kp] == pt).all()
    kp, pt = g["kept"]  # it held one with observations
    assert (flags[J["frame_mp"][kp]] & tr.HAS_OBS).all() and (r.rows[0][kp] == J["frame_mp"][kp]).all()
    assert (r.point_flags[pt] == tr.PT_IN_VIEW).all()  # visible, and matched nowhere
    assert not np.isin(pt, r.rows[0]).any()
    assert r.n_to_match >= 3 and r.nsearch == len(g["new"][0]) + len(g["wide"][0]) + len(g["reassign"][0])


def test_local_reference_outliers_thresholds_and_counting():
    """passes without the new entry points: it asserts on the reference"""
    a, b, c = lref("a"), lref("b"), lref("c")
    kp, _ = lbatch("a")["jobs"][0]["groups"]["out"]  # not stereo: the outliers keep their points
    assert a[0].rows[2][kp].all() and (a[0].rows[1][kp] >= 0).all() and a[0].rows[2].sum() == len(kp)
    kp, _ = lbatch("b")["jobs"][0]["groups"]["out"]  # stereo: nulled
    assert lbatch("b")["jobs"][0]["stereo"] == 1 and b[0].rows[2][kp].all() and (b[0].rows[1][kp] == -1).all()
    assert (b[0].rows[0][kp] >= 0).all()
    # 50 from both sides with recently_relocalised, 30 from both sides without
    assert (a[0].status, a[2].status) == (tr.OK, tr.LOST) and a[0].n_inliers >= 53 and 33 <= a[2].n_inliers <= 47
    assert (a[1].status, b[1].status) == (tr.OK, tr.LOST) and 33 <= a[1].n_inliers <= 47 and b[1].n_inliers <= 27
    assert [j["recently_relocalised"] for j in lbatch("a")["jobs"]] == [1, 0, 1]
    # only_tracking counts the points without observations, SLAM mode does not
    assert (b[2].status, c[2].status) == (tr.OK, tr.LOST) and b[2].n_inliers >= 33 and c[2].n_inliers <= 27
    assert b[2].opt.n_good == c[2].opt.n_good == 40
    # nToMatch == 0: no search, the optimisation still runs; n_local == 0
    assert (c[0].n_to_match, c[0].nsearch, c[0].opt.rounds, c[0].status) == (0, -1, 4, tr.OK)
    assert lbatch("c")["jobs"][0]["n_local"] == 50
    assert lbatch("c")["jobs"][1]["n_local"] == 0 and (c[1].n_to_match, c[1].nsearch, c[1].status) == (0, -1, tr.OK)


def test_local_reference_th_1_3_5():
    """passes without the new entry points: it asserts on the reference"""
    b = lbatch("a")
    assert [j["th"] for j in b["jobs"]] == [1.0, 3.0, 5.0]
    for j, narrower in ((1, 1.0), (2, 3.0)):  # the window of the smaller th misses what this one finds
        small = dict(b, jobs=[dict(J, th=narrower) if i == j else J for i, J in enumerate(b["jobs"])])
        assert tr.track_local(small, j).nsearch <= lref("a")[j].nsearch - 3, j


@functools.lru_cache(maxsize=None)
def chain_first():
    return ts.initial_batch([dict(groups=[G(60), G(10, shift_px=6.0)])], seed=62)


@functools.lru_cache(maxsize=None)
def chain_reference():
    """call 1 of the chained frame, then call 2 from its rows and pose with and without ORBGPU_PT_LAST_SEEN"""
    r1 = tr.track_initial(chain_first(), 0)
    marked, forgot = (ts.chain_local(chain_first(), 0, r1.rows, mark_culled=m) for m in (True, False))
    return r1, marked, tr.track_local(marked, 0, Tcw=r1.Tcw), forgot, tr.track_local(forgot, 0, Tcw=r1.Tcw)


def test_chain_reference_skips_the_points_call_1_culled():
    """passes without the new entry points: it asserts on the reference.  The cull of call 1 sets mnLastFrameSeen
    (Tracking.cpp:1183), so SearchLocalPoints skips those points at :1531 although the frame no longer holds
    them: in the local map, inside the frustum, yet neither counted in nToMatch nor matched, and without
    IncreaseVisible."""
    r1, marked, r, forgot, rf = chain_reference()
    assert r1.status == tr.OK and tr.decisive(r1) is None and tr.decisive(r) is None
    kp, pt = marked["jobs"][0]["groups"]["culled"]
    assert len(pt) >= 3 and (marked["jobs"][0]["frame_mp"][kp] == -1).all()
    assert (marked["jobs"][0]["table"]["flags"][pt] & tr.LAST_SEEN).all() and (pt < marked["jobs"][0]["n_local"]).all()
    assert r.in_frustum[pt].all() and not r.point_flags[pt].any() and not np.isin(pt, r.rows[0]).any()
    # the scene can tell: without the flag every one of them is projected and matched again
    assert rf.n_to_match == r.n_to_match + len(pt) and np.isin(pt, rf.rows[0]).all()
    assert (rf.point_flags[pt] == tr.PT_IN_VIEW).all() and rf.nsearch >= r.nsearch + len(pt)


# ---- CPU: UpdateLastFrame -------------------------------------------------------

def _depth_cases():
    rng = np.random.default_rng(51)
    out = []
    for n_pos in (99, 100, 101, 102):
        for m in (0, 99, 100, 101, n_pos):
            m = min(m, n_pos)
            z = np.concatenate([rng.uniform(0.5, 3.0, m), rng.uniform(3.5, 9.0, n_pos - m), [0.0, -1.0, np.nan] * 3])
            out.append((f"n_pos{n_pos}_m{m}_{len(out)}", rng.permutation(z).astype(np.float32), 3.2))
    z = np.concatenate([rng.uniform(0.5, 3.0, 98), np.full(8, 5.0), rng.uniform(6, 9, 10)])  # equal depths on the cut:
    out.append(("ties", rng.permutation(z).astype(np.float32), 3.2))                          # the index decides
    z = np.concatenate([rng.uniform(0.5, 3.0, 120), np.full(6, 3.5), rng.uniform(6, 9, 10)])
    out.append(("ties_after_m", rng.permutation(z).astype(np.float32), 3.2))
    z = np.concatenate([rng.uniform(0.5, 9.0, 150), [0.0, -0.0, -2.0, np.inf, np.inf, -np.inf, np.nan, np.nan]])
    out.append(("specials", rng.permutation(z).astype(np.float32), 3.2))
    out.append(("inf_only", np.array([np.inf] * 5 + [np.nan, 0.0], np.float32), 3.2))
    out.append(("none", np.array([0.0, -1.0, np.nan], np.float32), 3.2))
    out.append(("nan_th", rng.uniform(0.5, 9.0, 140).astype(np.float32), np.nan))
    return out


@functools.lru_cache(maxsize=None)
def last_frame_cases():
    rng = np.random.default_rng(52)
    cases = []
    for name, z, th in _depth_cases():
        pos = np.nonzero(z > 0)[0]
        held = rng.permutation(pos)[:len(pos) // 3]
        cases.append((name, ts.last_frame_case(rng, z, th, held_obs=held[::2], held_noobs=held[1::2])))
    return cases


def test_update_last_frame_closed_form_equals_the_literal_loop():
    """passes without the new entry points: it asserts on the reference"""
    rng = np.random.default_rng(53)
    cases = [c for _, c in last_frame_cases()]
    for _ in range(1000):
        n = int(rng.integers(0, 260))
        z = np.where(rng.random(n) < 0.8, rng.uniform(0.1, 9.0, n).round(int(rng.integers(0, 3))), 0.0)
        z = np.where(rng.random(n) < 0.2, rng.choice([0.0, -1.0, np.nan, np.inf, 2.0, 5.0], n), z)
        cases.append(ts.last_frame_case(rng, z, rng.choice([0.05, 3.2, 5.0, 20.0]),
                                        held_obs=np.nonzero(rng.random(n) < 0.3)[0]))
    seen_break = seen_all = 0
    for c in cases:
        want = tr.update_last_frame(c)
        vis = tr.visited_closed_form(c["depth"], c["th_depth"])
        assert len(vis) == want["n_visited"]
        create = np.zeros(len(c["depth"]), bool)
        create[vis] = True
        create &= ~((c["flags"] & 3) == 3)
        assert np.array_equal(create, want["created"].astype(bool))
        seen_break += want["n_visited"] < want["n_pos"]
        seen_all += want["n_visited"] == want["n_pos"] > 100
    assert seen_break > 50 and seen_all > 5


def test_update_last_frame_reference_cases():
    """passes without the new entry points: it asserts on the reference"""
    got = {name: tr.update_last_frame(c) for name, c in last_frame_cases()}
    assert len(got) == len(last_frame_cases()) == 26
    k = 0
    for n_pos in (99, 100, 101, 102):
        for m in (0, 99, 100, 101, n_pos):
            m = min(m, n_pos)
            assert got[f"n_pos{n_pos}_m{m}_{k}"]["n_visited"] == min(n_pos, max(m, 100) + 1), (n_pos, m)
            k += 1
    name, c = next(x for x in last_frame_cases() if x[0] == "ties")
    tied = np.nonzero(c["depth"] == 5.0)[0]  # visited: 98 close, then the tied by index up to the 101st
    r = got["ties"]
    assert r["n_visited"] == 101
    free = ~((c["flags"][tied] & 3) == 3)
    assert np.array_equal(r["created"][tied].astype(bool), free & (np.arange(8) < 3))
    assert got["specials"]["n_pos"] == int((last_frame_cases()[22][1]["depth"] > 0).sum())
    assert got["inf_only"]["n_visited"] == 5 and got["none"]["n_visited"] == 0 and got["none"]["n_created"] == 0
    assert got["nan_th"]["n_visited"] == 140  # z > NaN never ends the loop
    for name, c in last_frame_cases():  # a slot with observations is kept, one without is recreated
        r = got[name]
        obs = (c["flags"] & 3) == 3
        assert not r["created"][obs].any() and np.array_equal(r["flags"][obs], c["flags"][obs])
        made = r["created"].astype(bool)
        assert (r["flags"][made] == tr.VALID).all() and np.array_equal(r["mp_desc"][made], c["desc"][made])
        assert np.array_equal(r["pos"][~made], c["pos"][~made])
    assert any((r["created"].astype(bool) & (c["flags"] == tr.VALID)).any() for (_, c), r in
               zip(last_frame_cases(), got.values()))


# ---- CPU: the entry points' host side --------------------------------------------

def test_argument_errors_come_before_the_device():
    import track
    L = track._lib()
    p = ctypes.c_void_p(256)  # never dereferenced

    def initial(n=1, nf=1, stride=8, jobs=p, ws=p, res=p, rows=p):
        return L.orbgpu_track_initial_batch_device(n, jobs, nf, p, stride, ws, res, rows, None)

    for kw in (dict(n=-1), dict(nf=-1), dict(stride=0), dict(jobs=None), dict(ws=None), dict(res=None), dict(rows=None),
               dict(n=1 << 20, stride=1 << 12)):
        assert initial(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    assert initial(n=0, jobs=None, ws=None, res=None, rows=None) == 0  # nothing to do: no device needed

    def local(n=1, nf=1, stride=8, ps=8, jobs=p, ws=p, rows=p, flags=p):
        return L.orbgpu_track_local_map_batch_device(n, jobs, nf, p, stride, ps, ws, p, rows, flags, None)

    for kw in (dict(n=-1), dict(nf=-1), dict(stride=0), dict(ps=0), dict(jobs=None), dict(ws=None), dict(rows=None),
               dict(flags=None), dict(n=1 << 20, stride=1 << 12), dict(n=1 << 20, ps=1 << 12)):
        assert local(**kw) == -1, kw
    assert local(n=0, jobs=None, ws=None, rows=None, flags=None) == 0

    def update(n=1, stride=8, jobs=p, res=p, created=p):
        return L.orbgpu_update_last_frame_batch_device(n, jobs, stride, res, created, None)

    for kw in (dict(n=-1), dict(stride=0), dict(jobs=None), dict(res=None), dict(created=None),
               dict(n=1 << 20, stride=1 << 12)):
        assert update(**kw) == -1, kw
    assert update(n=0, jobs=None, res=None, created=None) == 0
    assert L.orbgpu_track_initial_workspace_bytes(3, 300) > 0
    assert L.orbgpu_track_local_workspace_bytes(3, 300, 240) > 0


@pytest.fixture(scope="module")
def track_args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("track_args") / "track_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2", "-std=c++17", "-Wall",
                    "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "track_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(track_args_main):
    """argument checks and the carving of both opaque blocks from a null base, compiled for the host with
    -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(track_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layouts_equal_the_header(track_args_main):
    import track
    r = subprocess.run([str(track_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = dict(re.findall(r"(\S+) (\d+)", r.stdout))
    want = {"orbgpu_track_initial_job": ctypes.sizeof(track.TrackInitialJob),
            "orbgpu_track_initial_result": ctypes.sizeof(track.TrackInitialResult),
            "orbgpu_track_local_job": ctypes.sizeof(track.TrackLocalJob),
            "orbgpu_track_local_result": ctypes.sizeof(track.TrackLocalResult),
            "orbgpu_update_last_frame_job": ctypes.sizeof(track.UpdateLastFrameJob),
            "orbgpu_update_last_frame_result": ctypes.sizeof(track.UpdateLastFrameResult),
            "initial_job.Tcw_init": track.TrackInitialJob.Tcw_init.offset,
            "initial_job.points": track.TrackInitialJob.points.offset,
            "initial_job.bow_nmatches": track.TrackInitialJob.bow_nmatches.offset,
            "initial_result.opt": track.TrackInitialResult.opt.offset,
            "initial_result.Tcw": track.TrackInitialResult.Tcw.offset,
            "local_job.Tcw": track.TrackLocalJob.Tcw.offset,
            "local_job.points": track.TrackLocalJob.points.offset,
            "local_result.Tcw": track.TrackLocalResult.Tcw.offset,
            "update_job.Rwc": track.UpdateLastFrameJob.Rwc.offset,
            "update_job.flags": track.UpdateLastFrameJob.flags.offset}
    assert {k: int(v) for k, v in got.items()} == want


# ---- GPU -----------------------------------------------------------------------

def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def T4(a):
    return np.array(a, np.float32).reshape(4, 4)


def ulps(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(T4(got).astype(np.float64) - want).max() / (ULP * max(1.0, float(np.abs(want).max()))))


def gpu_step(batch, stride=None, counts=None):
    import reloc
    import track
    arrs = ts.frames_arrays(batch, stride, counts)
    return track.TrackStep(reloc.Frames(*arrs[:10], counts=arrs[10]))


def run_initial(torch, batch, order=None, stride=None, counts=None, edit=None, n_frames=None):
    """call 1 for the batch's jobs in `order` (default all); edit(k, job dict) changes job k before the upload.
    Returns (per job the result's bytes, rows (n, 2, stride), the results, the step)."""
    import track
    step = gpu_step(batch, stride, counts)
    jobs = []
    for k in (range(len(batch["jobs"])) if order is None else order):
        J = dict(batch["jobs"][k])
        J["table"] = track.PointTable(**J["table"])
        if edit:
            edit(k, J)
        jobs.append(J)
    step.initial(jobs, n_frames=n_frames)
    torch.cuda.synchronize()
    raw = bytes(step.d_initial_results.cpu().numpy())
    sz = ctypes.sizeof(track.TrackInitialResult)
    return [raw[i * sz:(i + 1) * sz] for i in range(len(jobs))], step.initial_rows().copy(), step.initial_results(), step


def run_local(torch, batch, order=None, stride=None, counts=None, edit=None, point_stride=None):
    import track
    step = gpu_step(batch, stride, counts)
    jobs = []
    for k in (range(len(batch["jobs"])) if order is None else order):
        J = dict(batch["jobs"][k])
        J["table"] = track.PointTable(**J["table"])
        if edit:
            edit(k, J)
        jobs.append(J)
    step.local_map(jobs, point_stride=point_stride or max(len(J["table"]["flags"]) for J in batch["jobs"]))
    torch.cuda.synchronize()
    raw = bytes(step.d_local_results.cpu().numpy())
    sz = ctypes.sizeof(track.TrackLocalResult)
    return ([raw[i * sz:(i + 1) * sz] for i in range(len(jobs))], step.local_rows().copy(), step.local_results(),
            step.point_flags().copy(), step)


def assert_initial(g, rows, r, where):
    assert (g.status, g.searches, list(g.nsearch), g.nmatches, g.nmatches_map, g.vo) == \
        (r.status, r.searches, r.nsearch, r.nmatches, r.nmatches_map, r.vo), where
    n = len(r.rows[0])
    for k in range(2):
        np.testing.assert_array_equal(rows[k, :n], r.rows[k], err_msg=str(where))
    assert (rows[:, n:] == -1).all()
    if r.opt is None:
        assert bytes(g.Tcw) == np.asarray(r.Tcw, np.float32).tobytes() and g.opt.rounds == 0 and not any(g.opt.Tcw)
        return 0.0
    assert (g.opt.n_good, g.opt.rounds) == (r.opt.n_good, r.opt.rounds), where
    assert bytes(g.Tcw) == bytes(g.opt.Tcw)
    dev = ulps(g.Tcw, r.Tcw)
    assert dev <= 2.0, (where, dev)
    return dev


def assert_local(g, rows, pf, r, where):
    assert (g.status, g.n_to_match, g.nsearch, g.n_inliers, g.opt.n_good, g.opt.rounds) == \
        (r.status, r.n_to_match, r.nsearch, r.n_inliers, r.opt.n_good, r.opt.rounds), where
    n = len(r.rows[0])
    for k in range(3):
        np.testing.assert_array_equal(rows[k, :n], r.rows[k], err_msg=str(where))
    assert (rows[:2, n:] == -1).all() and not rows[2, n:].any()
    np.testing.assert_array_equal(pf[:len(r.point_flags)], r.point_flags, err_msg=str(where))
    assert not pf[len(r.point_flags):].any()
    assert bytes(g.Tcw) == bytes(g.opt.Tcw)
    dev = ulps(g.Tcw, r.Tcw)
    assert dev <= 2.0, (where, dev)
    return dev


def test_library_has_the_track_entry_points():
    """fails without the feature: the library has no orbgpu_track_* / orbgpu_update_last_frame_* symbols"""
    import orbgpu
    L = orbgpu.lib()
    for name in ("orbgpu_track_initial_workspace_bytes", "orbgpu_track_initial_batch_device",
                 "orbgpu_track_local_workspace_bytes", "orbgpu_track_local_map_batch_device",
                 "orbgpu_update_last_frame_batch_device"):
        assert hasattr(L, name), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INITIAL))
def test_gpu_initial_equals_the_reference(name):
    torch = _gpu()
    _, rows, res, _ = run_initial(torch, ibatch(name))
    worst = max(assert_initial(res[j], rows[j], iref(name)[j], (name, j)) for j in range(3))
    print(f"initial {name}: largest pose deviation {worst:.3f} ulp")
    if name == "edges":
        assert [len(r.opt.gidx) for r in iref(name)] == [63, 64, 65]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOCAL))
def test_gpu_local_map_equals_the_reference(name):
    torch = _gpu()
    _, rows, res, pf, _ = run_local(torch, lbatch(name))
    worst = max(assert_local(res[j], rows[j], pf[j], lref(name)[j], (name, j)) for j in range(3))
    print(f"local {name}: largest pose deviation {worst:.3f} ulp")
    if name == "edges":
        assert [len(r.opt.gidx) for r in lref(name)] == [63, 64, 65]


@pytest.mark.gpu
def test_gpu_chain_local_map_reads_call_1_in_place_and_skips_what_it_culled():
    """One frame through both calls, call 2's input made from call 1's GPU rows (track_scene.chain_local): the
    points call 1 culled lie in the local map inside the frustum and carry ORBGPU_PT_LAST_SEEN, so they are
    neither counted in nToMatch nor matched.  Call 2 given &d_results[0].Tcw of call 1 gives the bytes of call 2
    given the same pose from a buffer of its own, and equals the reference fed those pose bits."""
    torch = _gpu()
    first = chain_first()
    _, rows1, res, step = run_initial(torch, first)
    want1 = chain_reference()[0]
    assert_initial(res[0], rows1[0], want1, "chain, call 1")
    second = ts.chain_local(first, 0, rows1[0])
    pose = T4(res[0].Tcw)
    ptr = step.initial_pose_ptr(0)
    in_place = run_local(torch, second, edit=lambda k, J: J.update(Tcw=ptr))
    apart = run_local(torch, second, edit=lambda k, J: J.update(Tcw=pose))
    assert in_place[0] == apart[0] and np.array_equal(in_place[1], apart[1]) and np.array_equal(in_place[3], apart[3])
    r = tr.track_local(second, 0, Tcw=pose)
    assert tr.decisive(r) is None and r.status == tr.OK
    assert_local(in_place[2][0], in_place[1][0], in_place[3][0], r, "chain, call 2")
    kp, pt = second["jobs"][0]["groups"]["culled"]
    assert len(pt) >= 3 and not in_place[3][0][pt].any() and not np.isin(pt, in_place[1][0][0]).any()
    forgot = run_local(torch, ts.chain_local(first, 0, rows1[0], mark_culled=False),
                       edit=lambda k, J: J.update(Tcw=pose))  # without the flag they are projected and matched again
    assert forgot[2][0].n_to_match == in_place[2][0].n_to_match + len(pt) and np.isin(pt, forgot[1][0][0]).all()


@pytest.mark.gpu
def test_gpu_results_do_not_depend_on_the_batch_the_position_or_the_run():
    torch = _gpu()
    for run, batch in ((run_initial, ibatch("stereo")), (run_initial, ibatch("reference")), (run_local, lbatch("a"))):
        whole, again = run(torch, batch), run(torch, batch)
        assert whole[0] == again[0] and np.array_equal(whole[1], again[1])
        for q in range(3):
            others = [k for k in range(3) if k != q]
            alone, head, tail = run(torch, batch, order=[q]), run(torch, batch, order=[q] + others), \
                run(torch, batch, order=others + [q])
            for got, at in ((alone, 0), (head, 0), (tail, 2)):
                assert got[0][at] == whole[0][q], (q, at)
                np.testing.assert_array_equal(got[1][at], whole[1][q])
                if run is run_local:
                    np.testing.assert_array_equal(got[3][at], whole[3][q])


@pytest.mark.gpu
def test_gpu_over_capacity_frame_ends_alone():
    """A frame of 4097 keypoints -- one more than the projection matcher takes -- ends with CAPACITY in both
    calls; nothing is truncated and its neighbours' bytes are those of the run in which it has 300."""
    torch = _gpu()
    S = 4097
    for run, batch in ((run_initial, ibatch("mono")), (run_local, lbatch("a"))):
        clean = run(torch, batch, stride=S)
        got = run(torch, batch, stride=S, counts=[ts.N_KP, S, ts.N_KP])
        g = got[2][1]
        assert g.status == tr.CAPACITY and not any(g.Tcw) and g.opt.rounds == 0
        assert (got[1][1][:2] == -1).all()
        for k in (0, 2):
            assert got[0][k] == clean[0][k], k
            np.testing.assert_array_equal(got[1][k], clean[1][k])
    over = run_initial(torch, ibatch("mono"), stride=ts.N_KP, counts=[ts.N_KP, ts.N_KP + 1, ts.N_KP])  # more than stride
    assert over[2][1].status == tr.CAPACITY and over[2][0].status == tr.OK
    few = run_local(torch, lbatch("a"), point_stride=200)  # frame 0's table has 240 entries
    assert [r.status for r in few[2]] == [tr.CAPACITY, tr.OK, tr.LOST]


@pytest.mark.gpu
def test_gpu_bad_job_and_nan_pose_end_alone():
    torch = _gpu()
    nan = np.full((4, 4), np.nan, np.float32)
    clean = run_initial(torch, ibatch("mono"))
    for edit, status in ((lambda k, J: J.update(mode=7) if k == 1 else None, tr.BAD_JOB),
                         (lambda k, J: J.update(frame=3) if k == 1 else None, tr.BAD_JOB),
                         (lambda k, J: J.update(frame=-1) if k == 1 else None, tr.BAD_JOB),
                         (lambda k, J: J.update(Tcw_init=nan) if k == 1 else None, tr.FEW_MATCHES)):
        got = run_initial(torch, ibatch("mono"), edit=edit)
        assert got[2][1].status == status and (got[1][1] == -1).all()
        for k in (0, 2):
            assert got[0][k] == clean[0][k] and np.array_equal(got[1][k], clean[1][k]), k
    cleanr = run_initial(torch, ibatch("reference"))
    got = run_initial(torch, ibatch("reference"), edit=lambda k, J: J.update(Tcw_init=nan) if k == 1 else None)
    assert got[2][1].status in (tr.OK, tr.LOST) and got[2][1].opt.rounds == 4  # the optimisation's own bound
    for k in (0, 2):
        assert got[0][k] == cleanr[0][k] and np.array_equal(got[1][k], cleanr[1][k]), k
    cleanl = run_local(torch, lbatch("a"))
    for edit, statuses in ((lambda k, J: J.update(frame=3) if k == 1 else None, (tr.BAD_JOB,)),
                           (lambda k, J: J.update(n_local=10 ** 6) if k == 1 else None, (tr.BAD_JOB,)),
                           (lambda k, J: J.update(Tcw=nan) if k == 1 else None, (tr.OK, tr.LOST))):
        got = run_local(torch, lbatch("a"), edit=edit)
        assert got[2][1].status in statuses
        for k in (0, 2):
            assert got[0][k] == cleanl[0][k] and np.array_equal(got[1][k], cleanl[1][k]), k
            assert np.array_equal(got[3][k], cleanl[3][k])


@pytest.mark.gpu
def test_gpu_update_last_frame_equals_the_literal_loop():
    """d_created, the flags and the descriptors byte-equal, created positions bit-equal to the restated
    UnprojectStereo, untouched slots untouched; the same bytes alone, in a batch and again."""
    _gpu()
    import track
    cases = [c for _, c in last_frame_cases()]
    rng = np.random.default_rng(54)
    big = rng.uniform(0.3, 12.0, 1500).astype(np.float32)  # more than one pass of the block over the slots
    big[rng.random(1500) < 0.2] = 0.0
    cases.append(ts.last_frame_case(rng, big, 3.2, held_obs=np.nonzero(rng.random(1500) < 0.3)[0]))
    got = track.update_last_frame(cases)
    for k, (c, g) in enumerate(zip(cases, got)):
        want = tr.update_last_frame(c)
        assert (g["status"], g["n_created"], g["n_pos"], g["n_visited"]) == \
            (tr.OK, want["n_created"], want["n_pos"], want["n_visited"]), k
        n = len(c["depth"])
        assert g["created"][:n].tobytes() == want["created"].tobytes(), k
        assert g["flags"].tobytes() == want["flags"].tobytes() and g["mp_desc"].tobytes() == want["mp_desc"].tobytes(), k
        assert g["pos"].tobytes() == want["pos"].tobytes(), k
    again = track.update_last_frame(cases)
    alone = track.update_last_frame([cases[20]], stride=max(len(c["depth"]) for c in cases))
    for key in ("created", "flags", "pos", "mp_desc"):
        assert all(a[key].tobytes() == b[key].tobytes() for a, b in zip(got, again))
        assert alone[0][key].tobytes() == got[20][key].tobytes()
    over = track.update_last_frame([cases[0], dict(cases[1], n=4097), cases[2]], stride=4097)
    assert [r["status"] for r in over] == [tr.OK, tr.CAPACITY, tr.OK]
    assert not over[1]["created"].any() and over[1]["flags"].tobytes() == cases[1]["flags"].tobytes()
    for k in (0, 2):
        assert all(over[k][key].tobytes() == got[k][key].tobytes() for key in ("created", "flags", "pos", "mp_desc"))
