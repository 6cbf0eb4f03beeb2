"""LocalBundleAdjustment from the map mirror (include/orbgpu_localba_map.h,
csrc/localba_map.hip): the gather and the collection against
tests/localba_map_ref.py on tests/localba_map_scene.py's constructed maps.

CPU: the restatement itself on every named scene -- a bad covisible that
observes local points, a bad fixed observer, a bad pKF, first occurrences, a
slot without an observation, obs_idx beside the slot, a point without
observations, mono and stereo interleaved, a fixed camera first seen through a
late observation, kf_first local and fixed, the empty neighbourhood -- and its
arrays for converted tests/test_localba.py scenes against the arrays those
scenes were built from.  Without a device: the exported symbols (fails without
the feature), argument errors before the device, the stand-alone host program
under the address and undefined-behaviour sanitizers
(tests/cpp/localba_map_args_main.cpp), the struct layouts.

GPU: every int and every byte of every output equal to the restatement with
guard bytes past every count intact; the edge sizes; independence of the batch,
the position and the run; CAPACITY and BAD_JOB jobs ending alone, through the
following orbgpu_local_ba_batch_device and the collection too; gather -> LBA ->
collect on one stream against the same LBA call on the restatement's arrays.
No tolerances: integers and copied bytes, and orbgpu_localba.h promises
bit-repeatable, position-independent outputs.
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

import localba_map_ref as lr
import localba_map_scene as ls
import test_localba as tl

ROOT = Path(__file__).resolve().parent.parent
GUARD = 0x5A
BIG = dict(kf_stride=16, pose_stride=24, point_stride=64, edge_stride=128)  # every named scene fits
# a stereo / mono mix with injected outliers, every camera seeing every point
MIX = dict(n_local=3, n_fixed=2, n_points=30, seed=91, stereo=0.5, outliers=0.1, see=1.0)


@functools.lru_cache(maxsize=None)
def scene(name):
    return ls.SCENES[name]()


def ref(sc, kf=None, **strides):
    return lr.gather(sc["mirror"], sc["ba"], sc["kf"] if kf is None else kf, **dict(BIG, **strides))


def edges_of(r, kf=None, pt=None):
    """indices of the gathered edges from keyframe kf / of the mirror point pt"""
    ok = np.ones(r.n_edges, bool)
    if kf is not None:
        ok &= r.edge_kf == kf
    if pt is not None:
        ok &= np.array([r.local_points[m] == pt for m in r.edge_point], bool).reshape(r.n_edges)
    return np.nonzero(ok)[0]


# ---- CPU: the restatement on the named scenes ------------------------------------------------------------

def test_local_keyframes_bad_covisible_and_bad_pkf():
    """passes without the feature: it asserts on the restatement"""
    sc = scene("rich")
    nm, r = sc["names"], ref(sc)
    assert r.status == lr.OK and r.local_kfs == [nm["a"], nm["b"], nm["c"]]
    # the bad covisible observes local points, and is neither local nor fixed and has no edge
    assert all(nm["cb"] in sc["mirror"]["obs"][p] for p in nm["own"] + [nm["mix"]])
    assert nm["cb"] not in r.local_kfs + r.fixed_kfs and len(edges_of(r, kf=nm["cb"])) == 0
    # a bad fixed observer likewise
    assert nm["fb"] in sc["mirror"]["obs"][nm["mix"]] and nm["fb"] not in r.fixed_kfs and len(edges_of(r, kf=nm["fb"])) == 0
    assert nm["far"] not in r.local_kfs + r.fixed_kfs
    sc = scene("bad_pkf")
    nm, r = sc["names"], ref(sc)
    assert sc["mirror"]["kf_bad"][nm["a"]] and r.local_kfs == [nm["a"], nm["b"]] and r.fixed_kfs == [nm["d"]]
    assert r.local_points == nm["pts"] and len(edges_of(r, kf=nm["a"])) == 0 and r.n_edges == 5
    assert r.fixed.tolist() == [0, 0, 1]  # a bad pKF is still a free pose
    sc = scene("dup_covis")
    nm, r = sc["names"], ref(sc)
    assert r.local_kfs == [nm["a"], nm["b"], nm["c"]] and r.n_fixed == 0 and r.n_points == 3


def test_local_points_first_occurrence_and_slots():
    """passes without the feature: it asserts on the restatement"""
    sc = scene("rich")
    nm, r, M = sc["names"], ref(sc), sc["mirror"]
    lp = r.local_points
    assert len(set(lp)) == r.n_points and nm["dead"] not in lp and all(M["pt_flags"][p] & lr.VALID for p in lp)
    # `early`: c's slot number is the lower one, b is listed first: found in b, right after `tail`
    sb, sc_ = list(M["slots"][nm["b"]]).index(nm["early"]), list(M["slots"][nm["c"]]).index(nm["early"])
    assert sc_ < sb and lp.index(nm["early"]) == lp.index(nm["tail"]) + 1 < lp.index(nm["c_own"])
    # pKF's points come first, in slot order
    assert lp[:len([p for p in M["slots"][nm["a"]] if p >= 0 and p != nm["dead"]])] == \
        [int(p) for p in M["slots"][nm["a"]] if p >= 0 and p != nm["dead"]]
    # `ghost` is local through c's slot, lists no observation from c: no edge there, one from f0
    assert nm["ghost"] in lp and nm["c"] not in M["obs"][nm["ghost"]]
    assert r.edge_kf[edges_of(r, pt=nm["ghost"])].tolist() == [nm["f0"]]
    # `shift`: found in b's slot `held`, its edge takes the keypoint `shifted`
    e, = edges_of(r, pt=nm["shift"])
    kp = sc["ba"]["kp_obs"][nm["b"]]
    assert M["slots"][nm["b"]][nm["held"]] == nm["shift"] and M["slots"][nm["b"]][nm["shifted"]] == -1
    assert r.edge_slot[e] == nm["shifted"] != nm["held"] and r.obs[e].tobytes() == kp[nm["shifted"]].tobytes()
    assert r.obs[e].tobytes() != kp[nm["held"]].tobytes()
    assert r.inv_sigma2[e] == sc["ba"]["kp_inv_sigma2"][nm["b"]][nm["shifted"]]
    # a point without observations is a point with no edge
    assert nm["lonely"] in lp and len(edges_of(r, pt=nm["lonely"])) == 0
    assert (np.diff(r.edge_point) >= 0).all()


def test_fixed_cameras_edges_and_kf_first():
    """passes without the feature: it asserts on the restatement"""
    sc = scene("rich")
    nm, r = sc["names"], ref(sc)
    # e is first seen through the third observation of point 0, d through the first of point 1: e comes first
    assert r.local_points[:2] == [nm["p0"], nm["p1"]] and sc["mirror"]["obs"][nm["p0"]][-1] == nm["e"]
    assert r.fixed_kfs == [nm["e"], nm["d"], nm["f0"]]
    # mono and stereo interleaved in one point, in obs[] order without the bad keyframes
    e = edges_of(r, pt=nm["mix"])
    assert r.edge_kf[e].tolist() == [nm["a"], nm["b"], nm["c"], nm["d"], nm["e"]]
    assert (r.obs[e, 2] < 0).tolist() == [True, False, True, False, True]
    assert (r.obs[e, 2][r.obs[e, 2] < 0] == -1.0).all() and r.n_mono + r.n_stereo == r.n_edges and r.n_mono and r.n_stereo
    pose = {k: i for i, k in enumerate(r.local_kfs + r.fixed_kfs)}
    assert r.edge_pose[e].tolist() == [pose[k] for k in r.edge_kf[e]] and pose[nm["d"]] == r.n_local + 1
    # every negative mvuRight is written as -1.0f
    raw = np.concatenate([sc["ba"]["kp_obs"][k][:, 2] for k in range(len(sc["ba"]["kp_obs"]))])
    assert (raw < -1.5).any()
    # the map's first keyframe as a fixed camera, and (first_local) as a local pose with its flag set
    assert r.fixed.tolist() == [0, 0, 0, 1, 1, 1] and sc["ba"]["kf_first"][nm["f0"]]
    assert r.Tcw[pose[nm["f0"]]].tobytes() == sc["ba"]["kf_Tcw"][nm["f0"]].tobytes()
    sc = scene("first_local")
    nm, r = sc["names"], ref(sc)
    assert r.local_kfs == [nm["a"], nm["k0"]] and r.fixed_kfs == [nm["d"]] and r.fixed.tolist() == [0, 1, 1]
    assert r.n_edges == 9 and r.cam[1].tobytes() == sc["ba"]["kf_cam"][nm["k0"]].tobytes()
    sc = scene("empty")
    r = ref(sc)
    assert (r.status, r.n_local, r.n_fixed, r.n_points, r.n_edges, r.counts) == (lr.OK, 1, 0, 0, 0, (1, 1, 0, 0))


def test_capacity_and_bad_jobs_in_the_restatement():
    """passes without the feature: it asserts on the restatement"""
    sc = scene("rich")
    r = ref(sc)
    for name, count in (("kf_stride", r.n_local), ("pose_stride", r.n_local + r.n_fixed), ("point_stride", r.n_points),
                        ("edge_stride", r.n_edges)):
        assert ref(sc, **{name: count}).status == lr.OK
        c = ref(sc, **{name: count - 1})
        assert c.status == lr.CAPACITY and c.counts == (-1,) * 4
        assert (c.n_local, c.n_fixed, c.n_points, c.n_edges, c.n_mono) == (r.n_local, r.n_fixed, r.n_points, r.n_edges, r.n_mono)
    c = ref(sc, pose_stride=r.n_local + 1)
    assert c.fixed_kfs == r.fixed_kfs[:1] and len(c.Tcw) == r.n_local + 1 and c.local_kfs == r.local_kfs
    for what, b in bad_maps():
        assert lr.gather(b["mirror"], b["ba"], b["kf"], **BIG).status == lr.BAD_JOB, what
    assert lr.collect(c, np.ones(c.n_edges)) == []


CONVERTED = [tl.SIZES[k] for k in ("p1", "p2", "p16_e64", "e63", "e65")] + [MIX]


@pytest.mark.parametrize("kw", CONVERTED, ids=lambda kw: f"seed{kw['seed']}")
def test_converted_scene_gathers_to_the_arrays_it_was_built_from(kw):
    """passes without the feature: it asserts on the restatement.  Up to the documented orders: the points in
    first-seen order over the local keyframes' slots, the fixed poses in first-sight order."""
    s = tl.scene(**kw)
    sc = ls.from_problem(s)
    P, M, E, NL = len(s["Tcw"]), len(s["Xw"]), len(s["obs"]), s["n_local"]
    r = lr.gather(sc["mirror"], sc["ba"], sc["kf"], P, P, max(M, 1), max(E, 1))
    poses = r.local_kfs + r.fixed_kfs
    assert r.status == lr.OK and r.local_kfs == list(range(NL)) and sorted(poses) == list(range(P))
    assert sorted(r.local_points) == list(range(M)) and r.n_edges == E
    assert r.n_mono == int((s["obs"][:, 2] < 0).sum())
    assert r.Tcw.tobytes() == s["Tcw"][poses][:, :3].tobytes() and r.cam.tobytes() == s["cam"][poses].tobytes()
    assert r.fixed.tolist() == s["fixed"][poses].tolist() and r.Xw.tobytes() == s["Xw"][r.local_points].tobytes()
    vertex = {k: i for i, k in enumerate(poses)}
    at = 0
    for m, q in enumerate(r.local_points):  # a point's edges in the scene's order
        sel = np.nonzero(s["point_idx"] == q)[0]
        mine = slice(at, at + len(sel))
        assert (r.edge_point[mine] == m).all() and r.edge_pose[mine].tolist() == [vertex[int(k)] for k in s["pose_idx"][sel]]
        assert r.obs[mine].tobytes() == s["obs"][sel].tobytes() and r.inv_sigma2[mine].tobytes() == s["inv_sigma2"][sel].tobytes()
        at += len(sel)
    assert at == E


# ---- without a GPU: the entry points' host side --------------------------------------------------------

def test_library_has_the_gather_and_collect_entry_points():
    """fails without the feature: the library has no orbgpu_local_ba_gather_* / _collect_* symbols"""
    import orbgpu
    L = orbgpu.lib()
    for name in ("orbgpu_local_ba_gather_workspace_bytes", "orbgpu_local_ba_gather_batch_device",
                 "orbgpu_local_ba_collect_batch_device"):
        assert hasattr(L, name), name


def test_argument_errors_come_before_the_device():
    import localba
    import track
    L = localba._map_lib()
    p = ctypes.c_void_p(256)  # never dereferenced

    def mirror(**kw):
        m = track.MapMirrorStruct()
        m.n_kf, m.n_pt, m.n_slots_total, m.n_children_total, m.n_obs_total = 2, 3, 4, 1, 3
        for name, _ in track.MapMirrorStruct._fields_[6:]:
            setattr(m, name, 256)
        for k, v in kw.items():
            setattr(m, k, v)
        return ctypes.byref(m)

    def mirror_ba(**kw):
        b = localba.MapMirrorBAStruct()
        b.n_covis_all_total = 2
        for name, _ in localba.MapMirrorBAStruct._fields_[2:]:
            setattr(b, name, 256)
        for k, v in kw.items():
            setattr(b, k, v)
        return ctypes.byref(b)

    def gather(n=1, jobs=p, m=None, b=None, strides=(8, 8, 8, 8), null=None):
        ptrs = [p] * 16
        if null is not None:
            ptrs[null] = None
        return L.orbgpu_local_ba_gather_batch_device(n, jobs, m if m is not None else mirror(),
                                                     b if b is not None else mirror_ba(), *strides, *ptrs, None)

    bad = [dict(n=-1), dict(jobs=None), dict(m=mirror(n_kf=-1)), dict(m=mirror(n_obs_total=-1)), dict(m=mirror(kf_bad=None)),
           dict(m=mirror(slots=None)), dict(m=mirror(obs=None)), dict(m=mirror(pos=None)), dict(b=mirror_ba(n_covis_all_total=-1)),
           dict(b=mirror_ba(covis_all=None)), dict(b=mirror_ba(kf_first=None)), dict(b=mirror_ba(kf_Tcw=None)),
           dict(b=mirror_ba(kp_obs=None)), dict(b=mirror_ba(obs_idx=None))]
    bad += [dict(strides=tuple(0 if i == j else 8 for i in range(4))) for j in range(4)]
    bad += [dict(n=1 << 20, strides=tuple(1 << 12 if i == j else 8 for i in range(4))) for j in range(4)]
    bad += [dict(null=i) for i in range(16)]
    for kw in bad:
        assert gather(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    assert L.orbgpu_local_ba_gather_batch_device(1, p, None, mirror_ba(), 8, 8, 8, 8, *[p] * 16, None) == -1
    assert L.orbgpu_local_ba_gather_batch_device(1, p, mirror(), None, 8, 8, 8, 8, *[p] * 16, None) == -1
    assert L.orbgpu_local_ba_gather_batch_device(0, None, None, None, 8, 8, 8, 8, *[None] * 16, None) == 0
    assert L.orbgpu_local_ba_gather_workspace_bytes(3, 50, 3000) > 0

    def collect(n=1, strides=(8, 8, 8), null=None, n_kf=4, n_pt=9, kf_Tcw=p, pos=p):
        ptrs = [p] * 12
        if null is not None:
            ptrs[null] = None
        return L.orbgpu_local_ba_collect_batch_device(n, ptrs[0], *strides, *ptrs[1:], n_kf, n_pt, kf_Tcw, pos, None)

    bad = [dict(n=-1), dict(n_kf=-1), dict(n_pt=-1), dict(n=1 << 20, strides=(8, 8, 1 << 12))]
    bad += [dict(strides=tuple(0 if i == j else 8 for i in range(3))) for j in range(3)]
    bad += [dict(null=i) for i in range(12)]  # Tcw_out (8) and Xw_out (9) are needed: kf_Tcw and pos are given
    for kw in bad:
        assert collect(**kw) == -1, kw
    assert L.orbgpu_local_ba_collect_batch_device(0, None, 8, 8, 8, *[None] * 11, 0, 0, None, None, None) == 0


@pytest.fixture(scope="module")
def args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("localba_map_args") / "localba_map_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "localba_map_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(args_main):
    """argument checks of both calls and the carving of the opaque block from a null base, compiled for the host
    with -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layouts_equal_the_header(args_main):
    import localba
    r = subprocess.run([str(args_main), "sizes"], capture_output=True, text=True, check=True)
    got = dict(re.findall(r"(\S+) (\d+)", r.stdout))
    B, J, R = localba.MapMirrorBAStruct, localba.GatherJob, localba.GatherResult
    want = {"orbgpu_map_mirror_ba": ctypes.sizeof(B), "orbgpu_localba_gather_job": ctypes.sizeof(J),
            "orbgpu_localba_gather_result": ctypes.sizeof(R), "orbgpu_localba_job": localba.JOB_DTYPE.itemsize,
            "ba.covis_all_offset": B.covis_all_offset.offset, "ba.kf_first": B.kf_first.offset, "ba.kp_obs": B.kp_obs.offset,
            "ba.obs_idx": B.obs_idx.offset, "result.n_fixed": R.n_fixed.offset, "result.n_stereo": R.n_stereo.offset}
    assert {k: int(v) for k, v in got.items()} == want
    assert localba.GATHER_RESULT_DTYPE.fields["n_stereo"][1] == R.n_stereo.offset


# ---- GPU ----------------------------------------------------------------------------------------------

def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def upload(sc):
    import localba
    import track
    return track.MapMirror(**sc["mirror"]), localba.MapMirrorBA(**sc["ba"])


# the gather's arrays: (name, columns, which stride counts its rows, the restatement's field)
ARRAYS = (("Tcw", 12, "pose"), ("fixed", 0, "pose"), ("cam", 5, "pose"), ("Xw", 3, "point"), ("edge_pose", 0, "edge"),
          ("edge_point", 0, "edge"), ("obs", 3, "edge"), ("inv_sigma2", 0, "edge"), ("local_kfs", 0, "kf"),
          ("fixed_kfs", 0, "pose"), ("local_points", 0, "point"), ("edge_kf", 0, "edge"), ("edge_slot", 0, "edge"))
LISTS = ("local_kfs", "fixed_kfs", "local_points", "edge_kf", "edge_slot")  # int[n][stride]
UNTOUCHED = ("Tcw_out", "Xw_out", "erase", "to_erase", "n_erase", "results")  # not the gather's to write


def guard_fill(torch, B):
    for name, t in B.t.items():
        if name not in ("gather_jobs", "ws"):
            t.view(torch.uint8).fill_(GUARD)  # the workspace need not be zeroed


def run_gather(torch, sc, kfs, d=None, **strides):
    """The gather for `kfs` on one map with every output buffer and the workspace filled with GUARD bytes first.
    Returns the localba.MapLocalBA, its buffers downloaded into .h"""
    import localba
    mirror, ba = d or upload(sc)
    B = localba.MapLocalBA(mirror, ba, kfs, **dict(BIG, **strides))
    guard_fill(torch, B)
    B.gather()
    torch.cuda.synchronize()
    B.h = {name: B.host(name) for name in B.t if name not in ("gather_ws", "gather_jobs")}
    return B


def guard(a):
    return (np.ascontiguousarray(a).view(np.uint8) == GUARD).all()


def job_rows(B, name, k, stride):
    """job k's range of a downloaded buffer, as rows"""
    a, S = B.h[name], B.strides[stride]
    return a[k] if name in LISTS else a[k * S:(k + 1) * S]


def assert_job(B, k, r, where):
    """job k of the run B against the restatement r: every int, every byte, and the guard bytes past them"""
    R = B.h["gather_results"][k]
    assert tuple(int(R[f]) for f in R.dtype.names) == (r.status, r.n_local, r.n_fixed, r.n_points, r.n_edges, r.n_mono,
                                                       r.n_stereo, 0), where
    J, S = B.h["jobs"][k], B.strides
    assert (J["n_poses"], J["n_local"], J["n_points"], J["n_edges"]) == r.counts, where
    assert (J["pose_offset"], J["point_offset"], J["edge_offset"], J["out_pose_offset"]) == \
        (k * S["pose"], k * S["point"], k * S["edge"], k * S["kf"]), where
    for name, cols, stride in ARRAYS:
        got = job_rows(B, name, k, stride)
        want = np.asarray(getattr(r, name), got.dtype).reshape((-1, cols) if cols else (-1,))
        assert len(want) <= len(got), (where, name)
        assert got[:len(want)].tobytes() == want.tobytes(), (where, name)
        assert guard(got[len(want):]), (where, name)  # entries past the counts are not written


def assert_untouched(B, where):
    for name in UNTOUCHED:
        assert guard(B.h[name]), (where, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ls.SCENES))
def test_gpu_named_scenes_equal_the_restatement(name):
    torch = _gpu()
    sc = scene(name)
    B = run_gather(torch, sc, [sc["kf"]])
    assert_job(B, 0, ref(sc), name)
    assert_untouched(B, name)


W = (0, 1, 63, 64, 65, 255, 256, 257)  # around the wave (a point's observations) and the workgroup (every stripe)
EDGE_SIZES = [("covis", dict(n_covis=w), lambda r, sc, w=w: r.n_local == 1 + sum(not sc["mirror"]["kf_bad"][k] for k in sc["names"]["cov"])
               and len(sc["names"]["cov"]) == w) for w in W + (1030,)]
EDGE_SIZES += [("slots", dict(n_points=w, nulls=0), lambda r, sc, w=w: len(sc["mirror"]["slots"][sc["kf"]]) == w == r.n_points)
               for w in W + (4100,)]
EDGE_SIZES += [("obs", dict(n_obs0=w), lambda r, sc, w=w: len(sc["mirror"]["obs"][sc["names"]["pts"][0]]) == w) for w in W]
EDGE_SIZES += [("fixed", dict(n_fixed=w), lambda r, sc, w=w: r.n_fixed == w) for w in W]


@pytest.mark.gpu
@pytest.mark.parametrize("what,kw,holds", EDGE_SIZES, ids=[f"{a}{list(b.values())[0]}" for a, b, _ in EDGE_SIZES])
def test_gpu_edge_sizes(what, kw, holds):
    """the covisible list, pKF's slots (and with them the local points), one point's observations and the fixed
    cameras at 0, 1, and one below, at and one above the wave and the workgroup; 1030 covisibles and 4100 points
    are more than one pass of the launches that stride over keyframes and points.  The strides fit exactly."""
    torch = _gpu()
    sc = ls.sized(**kw)
    r = lr.gather(sc["mirror"], sc["ba"], sc["kf"], 1 << 20, 1 << 20, 1 << 20, 1 << 20)
    assert r.status == lr.OK and holds(r, sc), (what, kw)
    strides = dict(kf_stride=r.n_local, pose_stride=r.n_local + r.n_fixed, point_stride=max(r.n_points, 1),
                   edge_stride=max(r.n_edges, 1))
    B = run_gather(torch, sc, [sc["kf"]], **strides)
    assert_job(B, 0, r, (what, kw))


def snap(B, k):
    return (B.h["gather_results"][k].tobytes(), tuple(int(B.h["jobs"][k][f]) for f in ("n_poses", "n_local", "n_points", "n_edges")),
            tuple(np.ascontiguousarray(job_rows(B, name, k, stride)).tobytes() for name, _, stride in ARRAYS))


@pytest.mark.gpu
def test_gpu_results_do_not_depend_on_the_batch_the_position_or_the_run():
    """five jobs on one shared map, two of them with the same pKF: the same bytes alone, first, last, in a second
    run and on the workspace the first run left behind"""
    torch = _gpu()
    sc = scene("rich")
    nm = sc["names"]
    kfs = [nm["a"], nm["b"], nm["a"], nm["far"], nm["f0"]]
    d = upload(sc)
    refs = [ref(sc, kf=k) for k in kfs]
    assert [r.status for r in refs] == [lr.OK] * 5 and len({r.n_points for r in refs}) >= 2
    whole = run_gather(torch, sc, kfs, d=d)
    for k in range(5):
        assert_job(whole, k, refs[k], k)
    assert snap(whole, 0) == snap(whole, 2)
    again = run_gather(torch, sc, kfs, d=d)
    whole.gather()  # on the workspace the first run left behind
    torch.cuda.synchronize()
    rerun = SimpleNamespace(h={name: whole.host(name) for name in whole.h}, strides=whole.strides, n=whole.n)
    for q in range(5):
        others = [k for k in range(5) if k != q]
        alone = run_gather(torch, sc, [kfs[q]], d=d)
        head = run_gather(torch, sc, [kfs[k] for k in [q] + others], d=d)
        tail = run_gather(torch, sc, [kfs[k] for k in others + [q]], d=d)
        for got, at in ((alone, 0), (head, 0), (tail, 4), (again, q), (rerun, q)):
            assert snap(got, at) == snap(whole, q), (q, at)


def bad_maps():
    """the `rich` map with one id out of range where pKF's job reads it: a covisible, a local keyframe's slot (two
    ways), a local point's observation (two ways), an edge's obs_idx (two ways); far's job reads none of them"""
    sc = scene("rich")
    nm, M, A = sc["names"], sc["mirror"], sc["ba"]
    n_kf, n_pt = len(M["kf_bad"]), len(M["pt_flags"])
    out = []

    def edit(key, which, at, v, ba=False):
        src = A if ba else M
        rows = [np.array(x).copy() for x in src[key]]
        rows[which][at] = v
        new = dict(src, **{key: [r if isinstance(src[key][0], np.ndarray) else r.tolist() for r in rows]})
        return dict(sc, ba=new) if ba else dict(sc, mirror=new)

    out.append(("covis n_kf", edit("covis_all", nm["a"], 2, n_kf, ba=True)))
    out.append(("covis -1", edit("covis_all", nm["a"], 0, -1, ba=True)))
    out.append(("slot n_pt", edit("slots", nm["c"], 1, n_pt)))
    out.append(("slot -2", edit("slots", nm["a"], 0, -2)))
    out.append(("obs n_kf", edit("obs", nm["mix"], 6, n_kf)))
    out.append(("obs -1", edit("obs", nm["p0"], 0, -1)))
    out.append(("obs_idx n_slots", edit("obs_idx", nm["shift"], 0, len(M["slots"][nm["b"]]), ba=True)))
    out.append(("obs_idx -1", edit("obs_idx", nm["ghost"], 0, -1, ba=True)))
    return out


def solve_and_collect(torch, B):
    """the following two calls on the gathered buffers; downloads again"""
    B.solve()
    B.collect()
    torch.cuda.synchronize()
    B.h = {name: B.host(name) for name in B.t if name not in ("gather_ws", "gather_jobs", "ws")}


def assert_rejected_alone(B, refs, where):
    """LBA reports rounds = -1 for exactly the jobs that are not OK and leaves their outputs alone; the collection
    gives n_erase = 0 for them and writes no entry"""
    S = B.strides
    for k, r in enumerate(refs):
        res = B.h["results"][k]
        out = (B.h["Tcw_out"][k * S["kf"]:(k + 1) * S["kf"]], B.h["Xw_out"][k * S["point"]:(k + 1) * S["point"]],
               B.h["erase"][k * S["edge"]:(k + 1) * S["edge"]])
        if r.status == lr.OK:
            assert res["rounds"] != -1, (where, k)
            assert not guard(out[0][:r.n_local]) and guard(out[0][r.n_local:]) and guard(out[1][r.n_points:]), (where, k)
            assert guard(out[2][r.n_edges:]), (where, k)
            assert 0 <= B.h["n_erase"][k] <= r.n_edges and guard(B.h["to_erase"][k][B.h["n_erase"][k]:]), (where, k)
        else:
            assert res["rounds"] == -1 and all(guard(o) for o in out), (where, k)
            assert B.h["n_erase"][k] == 0 and guard(B.h["to_erase"][k]), (where, k)


@pytest.mark.gpu
def test_gpu_capacity_for_each_stride_ends_alone():
    """each stride one below pKF's count (CAPACITY, true counts, the first `stride` entries) and at it (OK), in a
    batch with far's job, which fits everywhere; then LBA and the collection on the prepared jobs"""
    torch = _gpu()
    sc = scene("rich")
    nm, full = sc["names"], ref(sc)
    d = upload(sc)
    kfs = [nm["far"], nm["a"], nm["far"]]
    for name, count in (("kf_stride", full.n_local), ("pose_stride", full.n_local + full.n_fixed),
                        ("point_stride", full.n_points), ("edge_stride", full.n_edges)):
        for delta, want in ((-1, lr.CAPACITY), (0, lr.OK)):
            strides = {name: count + delta}
            refs = [ref(sc, kf=k, **strides) for k in kfs]
            assert [r.status for r in refs] == [lr.OK, want, lr.OK], (name, delta)
            B = run_gather(torch, sc, kfs, d=d, **strides)
            for k in range(3):
                assert_job(B, k, refs[k], (name, delta, k))
            solve_and_collect(torch, B)
            assert_rejected_alone(B, refs, (name, delta))
    refs = [ref(sc, kf=k, pose_stride=full.n_local + 1) for k in kfs]  # one fixed camera fits
    B = run_gather(torch, sc, kfs, d=d, pose_stride=full.n_local + 1)
    assert refs[1].status == lr.CAPACITY and len(refs[1].fixed_kfs) == 1
    for k in range(3):
        assert_job(B, k, refs[k], ("one fixed", k))


@pytest.mark.gpu
def test_gpu_bad_jobs_end_alone():
    """BAD_JOB through every kind of id the job reads (ordinary input: each is range-checked before it is used),
    in a batch with a job that never reads that id; then LBA and the collection on the prepared jobs"""
    torch = _gpu()
    sc = scene("rich")
    nm = sc["names"]
    n_kf = len(sc["mirror"]["kf_bad"])
    kfs = [nm["far"], n_kf, nm["a"], -1]  # pKF itself outside the map, twice
    refs = [ref(sc, kf=k) for k in kfs]
    assert [r.status for r in refs] == [lr.OK, lr.BAD_JOB, lr.OK, lr.BAD_JOB]
    B = run_gather(torch, sc, kfs)
    for k in range(4):
        assert_job(B, k, refs[k], ("kf", k))
    solve_and_collect(torch, B)
    assert_rejected_alone(B, refs, "kf")
    for what, bad in bad_maps():
        kfs = [nm["far"], nm["a"], nm["far"]]
        refs = [lr.gather(bad["mirror"], bad["ba"], k, **BIG) for k in kfs]
        assert [r.status for r in refs] == [lr.OK, lr.BAD_JOB, lr.OK], what
        B = run_gather(torch, bad, kfs)
        for k in range(3):
            assert_job(B, k, refs[k], (what, k))
        solve_and_collect(torch, B)
        assert_rejected_alone(B, refs, what)


@pytest.mark.gpu
def test_gpu_offsets_outside_their_arrays_are_bad_jobs():
    """an offset + count beyond its array, which the list-built maps cannot express: one word of the uploaded
    mirrors is overwritten for each -- pKF's covisible run, a local keyframe's and a fixed camera's slot run, a
    local point's observation run, by the offset and by the count; far's job reads none of them"""
    torch = _gpu()
    sc = scene("rich")
    nm = sc["names"]
    kfs = [nm["far"], nm["a"], nm["far"]]
    refs = [ref(sc, kf=nm["far"]), lr._bad_job(), ref(sc, kf=nm["far"])]
    big = 1 << 30
    for which, name, at, v in ((1, "covis_all_offset", nm["a"], big), (1, "n_covis_all", nm["a"], big), (1, "n_covis_all", nm["a"], -1),
                               (0, "slot_offset", nm["b"], big), (0, "n_slots", nm["c"], big), (0, "slot_offset", nm["d"], -1),
                               (0, "n_slots", nm["e"], -3), (0, "obs_offset", nm["mix"], big), (0, "n_obs", nm["p0"], big),
                               (0, "n_obs", nm["lonely"], -1)):
        d = upload(sc)
        d[which].t[name].view(torch.int32)[at] = v
        B = run_gather(torch, sc, kfs, d=d)
        for k in range(3):
            assert_job(B, k, refs[k], (name, at, v, k))


CHAIN = {"p1": tl.SIZES["p1"], "mix": MIX}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CHAIN))
def test_gpu_chain_is_three_calls_on_one_stream(name):
    """gather -> orbgpu_local_ba_batch_device -> collect enqueued on one non-default stream with no
    synchronisation between them, on a converted tests/test_localba.py scene: two jobs (pKF = pose 0, the scene's
    own job, and pKF = the last local pose).  Tcw_out, Xw_out, erase and the LBA result structs equal byte for
    byte the same device call on the restatement's arrays uploaded at the same offsets with the same totals and
    max_local; vToErase equals the restatement's; then one job alone with the mirror's arrays writable."""
    torch = _gpu()
    import localba
    s = tl.scene(**CHAIN[name])
    sc = ls.from_problem(s)
    P, M, E, NL = len(s["Tcw"]), len(s["Xw"]), len(s["obs"]), s["n_local"]
    strides = dict(kf_stride=NL + 1, pose_stride=P + 2, point_stride=M + 3, edge_stride=E + 5)
    kfs = [0, NL - 1]
    refs = [lr.gather(sc["mirror"], sc["ba"], k, **strides) for k in kfs]
    assert [r.status for r in refs] == [lr.OK, lr.OK] and refs[0].n_edges == E
    d = upload(sc)
    B = localba.MapLocalBA(*d, kfs, **strides)
    B.solve_workspace()
    guard_fill(torch, B)
    # the same LBA call on the restatement's arrays
    S = B.strides
    total = {"poses": 2 * S["pose"], "local": 2 * S["kf"], "points": 2 * S["point"], "edges": 2 * S["edge"]}
    host = {}
    for nm_, dtype, cols, tot in localba.INPUTS + localba.OUTPUTS:
        shape = (total[tot], cols) if cols else (total[tot],)
        host[nm_] = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, GUARD, np.uint8).view(dtype).reshape(shape)
    rows = []
    for k, r in enumerate(refs):
        po, lo, eo = k * S["pose"], k * S["point"], k * S["edge"]
        rows.append(r.counts + (po, lo, eo, k * S["kf"]))
        for nm_, stride0 in (("Tcw", po), ("fixed", po), ("cam", po), ("Xw", lo), ("edge_pose", eo), ("edge_point", eo),
                             ("obs", eo), ("inv_sigma2", eo)):
            host[nm_][stride0:stride0 + len(getattr(r, nm_))] = getattr(r, nm_)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    jobs = torch.from_numpy(localba.make_jobs(rows).view(np.uint8).reshape(2, 32)).cuda()
    want_res = torch.full((2, 32), GUARD, dtype=torch.uint8, device="cuda")
    ws = torch.zeros_like(B.t["ws"])
    localba.local_ba_batch_device(jobs, *(dev[n] for n, *_ in localba.INPUTS), *(dev[n] for n, *_ in localba.OUTPUTS),
                                  want_res, ws, S["kf"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    B.run(stream)
    stream.synchronize()
    B.h = {n: B.host(n) for n in B.t if n not in ("gather_ws", "gather_jobs", "ws")}
    for k in range(2):
        assert_job(B, k, refs[k], (name, k))
    for n, *_ in localba.OUTPUTS:
        assert B.h[n].tobytes() == dev[n].cpu().numpy().tobytes(), n
    assert B.h["results"].tobytes() == want_res.cpu().numpy().tobytes()
    assert [int(x) for x in B.h["results"]["rounds"]] == [2 if r.n_edges else 0 for r in refs]
    for k, r in enumerate(refs):
        erase = B.h["erase"][k * S["edge"]:k * S["edge"] + r.n_edges]
        want = lr.collect(r, erase)
        n = int(B.h["n_erase"][k])
        assert n == len(want) == int(B.h["results"]["n_erase"][k]), k
        assert [tuple(int(v) for v in row) for row in B.h["to_erase"][k][:n]] == want and guard(B.h["to_erase"][k][n:]), k
        if name == "mix" and k == 0:  # outliers flagged in both classes, the monocular ones first
            mono = [bool(sc["ba"]["kp_obs"][kf][slot][2] < 0) for kf, _, slot in want]
            assert any(mono) and not all(mono) and mono == sorted(mono, reverse=True)
    # one job with the mirror's own arrays writable: the rows of its keyframes and points are the outputs
    d = upload(sc)
    One = localba.MapLocalBA(*d, [0], **strides)
    One.solve_workspace()
    guard_fill(torch, One)
    before_T, before_X = d[1].t["kf_Tcw"].cpu().numpy().view(np.float32).reshape(-1, 12).copy(), \
        d[0].t["pos"].cpu().numpy().view(np.float32).reshape(-1, 3).copy()
    torch.cuda.synchronize()
    One.run(stream, write_mirror=True)
    stream.synchronize()
    r = refs[0]
    T_out, X_out = One.host("Tcw_out"), One.host("Xw_out")
    assert T_out[:r.n_local].tobytes() == B.h["Tcw_out"][:r.n_local].tobytes()  # position and batch independent
    after_T = d[1].t["kf_Tcw"].cpu().numpy().view(np.float32).reshape(-1, 12)
    after_X = d[0].t["pos"].cpu().numpy().view(np.float32).reshape(-1, 3)
    for i, kf in enumerate(r.local_kfs):
        assert after_T[kf].tobytes() == T_out[i, :12].tobytes(), kf
    for j, p in enumerate(r.local_points):
        assert after_X[p].tobytes() == X_out[j].tobytes(), p
    others = [k for k in range(P) if k not in r.local_kfs]
    assert after_T[others].tobytes() == before_T[others].tobytes()
    rest = [p for p in range(M) if p not in r.local_points]
    assert after_X[rest].tobytes() == before_X[rest].tobytes()
    if r.n_edges:
        assert after_T[r.local_kfs].tobytes() != before_T[r.local_kfs].tobytes()


@pytest.mark.gpu
def test_gpu_write_back_leaves_other_rows_alone():
    """the scatter of the collection on the `rich` map, where most keyframes and points are outside the job: rows
    of keyframes and points outside it keep their bytes, the job's rows are the outputs"""
    torch = _gpu()
    import localba
    sc = scene("rich")
    r = ref(sc)
    d = upload(sc)
    B = localba.MapLocalBA(*d, [sc["kf"]], **BIG)
    B.solve_workspace()
    guard_fill(torch, B)
    before_T, before_X = sc["ba"]["kf_Tcw"], sc["mirror"]["pos"]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    B.run(stream, write_mirror=True)
    stream.synchronize()
    T_out, X_out = B.host("Tcw_out"), B.host("Xw_out")
    after_T = d[1].t["kf_Tcw"].cpu().numpy().view(np.float32).reshape(-1, 12)
    after_X = d[0].t["pos"].cpu().numpy().view(np.float32).reshape(-1, 3)
    for kf in range(len(before_T)):
        want = T_out[r.local_kfs.index(kf), :12] if kf in r.local_kfs else before_T[kf]
        assert after_T[kf].tobytes() == want.tobytes(), kf
    for p in range(len(before_X)):
        want = X_out[r.local_points.index(p)] if p in r.local_points else before_X[p]
        assert after_X[p].tobytes() == want.tobytes(), p
    assert len(r.local_kfs) < len(before_T) and len(r.local_points) < len(before_X)
