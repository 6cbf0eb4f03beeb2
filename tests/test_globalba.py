"""Global bundle adjustment (include/orbgpu_globalba.h, csrc/globalba.hip,
include/orbslam2_amd/BundleAdjuster.h) against the numpy restatement of
Optimizer::BundleAdjustment (tests/globalba_ref.py).

Parity: every element of every pose within ULP_BOUND float32 ulps at the scale
max(1, max|.|) of that pose, every point coordinate within the same bound at
the scale max(1, max|.|) of the problem's points (tests/test_localba.py's
measure).  The kernels and the restatement sum a vertex's block, a block of the
reduced system and every entry of the factor in the same order, but associate
the robust chi2 and computeScale's sum differently, so the bound is measured,
not fixed (the rule of test_sim3opt.py): MEASURED_WORST is the largest
deviation the restatement shows on any fixture when its points are permuted and
its edges are permuted within each point (8 permutations each), and ULP_BOUND =
max(2, 4 x MEASURED_WORST).  test_ref_permutation_spread_of_every_fixture
asserts the measurement.

iterations, rejected, stopped and iterations_applied are compared for equality:
every fixture's seed and iteration count are chosen on the CPU so that every
chi2 decision of the restatement (accept or reject, rho == 0, the stop
criterion) stays 1e-6 (relative) from its threshold, under each of the 8
permutations too; the tests assert that (globalba_ref.decisive) before they
compare.

Measured on the CPU, the restatement under permutation: 0.000 ulp on each of the
25 fixtures, so the bound is the floor, 2 ulp.  Measured on an MI355X against
the restatement: 0.000 ulp on all 25 fixtures, on a non-default stream and
through the C++ adapter, with the four counters, n_free and the active points
equal everywhere; the stop flag set from a second thread landed
before the first, the second and the third iteration of the 20-iteration run.
"""
import ctypes
import functools
import os
import re
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import globalba
import globalba_ref as gr
import globalba_scene as gs
import lm_ref
import orbgpu
import poseopt_ref

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
ULP = 2.0 ** -23
PERMUTATIONS = 8
NB = 48  # csrc/globalba.hip: kNB, the panel width of the blocked Cholesky
# the restatement's worst deviation under 8 permutations of any fixture, measured on the CPU: 0.000 ulp on
# every fixture (the doubles differ, but nowhere across a float32 rounding boundary), so the bound is the
# floor
MEASURED_WORST = 0.0
ULP_BOUND = max(2.0, 4.0 * MEASURED_WORST)

ALL = dict(see=1.0)
# name: (scene, n_iterations, robust).  Free poses 6 F in {6, NB - 6, NB, NB + 6, 2 NB + 6} (pose 0 is
# fixed, so n_poses = F + 1); init_f1 is the monocular initial map (two keyframes, 150 points, 20
# iterations, robust); p70 has point 0 seen from all 70 poses (a run longer than a wave) and pose 1
# seeing all 260 points (more than 256 edges); m* are the point counts and e* the edge counts around the
# wave and the workgroup (e1: one edge to the fixed pose, so no free pose at all); mono only, stereo
# only, mixed; robust 0 and 1; gap: poses 0 and 4 fixed, free pose 2 without an edge between free poses
# that have some; all_fixed: the points alone
FIXTURES = {
    "init_f1": (dict(n_poses=2, n_points=150, seed=2501), 20, 1),
    "f7": (dict(n_poses=NB // 6, n_points=40, seed=2, stereo=0.5), 4, 1),
    "f8": (dict(n_poses=NB // 6 + 1, n_points=40, seed=3, stereo=1.0, drop_mono=True), 4, 0),
    "f9": (dict(n_poses=NB // 6 + 2, n_points=40, seed=4, stereo=0.3), 4, 1),
    "f17": (dict(n_poses=2 * NB // 6 + 2, n_points=60, seed=5, stereo=0.5), 4, 0),
    "p70": (dict(n_poses=70, n_points=260, seed=6, stereo=0.3, thin=(0.1, 0, 1), **ALL), 3, 0),
    "m0": (dict(n_poses=2, n_points=0, seed=10), 5, 1),
    "m1": (dict(n_poses=2, n_points=1, seed=11, stereo=1.0, **ALL), 3, 0),
    "m63": (dict(n_poses=2, n_points=63, seed=12, stereo=0.5, **ALL), 3, 1),
    "m64": (dict(n_poses=2, n_points=64, seed=13, stereo=1.0, drop_mono=True, **ALL), 3, 1),
    "m65": (dict(n_poses=2, n_points=65, seed=14, **ALL), 3, 1),
    "m255": (dict(n_poses=2, n_points=255, seed=15, stereo=0.5, **ALL), 3, 0),
    "m256": (dict(n_poses=2, n_points=256, seed=16, **ALL), 3, 1),
    "m257": (dict(n_poses=2, n_points=257, seed=17, stereo=1.0, **ALL), 3, 1),
    "e0": (dict(n_poses=3, n_points=5, seed=20, n_edges=0, **ALL), 5, 1),
    "e1": (dict(n_poses=3, n_points=90, seed=21, n_edges=1, stereo=1.0, **ALL), 3, 0),
    "e63": (dict(n_poses=3, n_points=90, seed=22, n_edges=63, stereo=0.5, **ALL), 3, 1),
    "e64": (dict(n_poses=3, n_points=90, seed=23, n_edges=64, stereo=0.5, **ALL), 3, 0),
    "e65": (dict(n_poses=3, n_points=90, seed=24, n_edges=65, stereo=0.5, **ALL), 3, 1),
    "e255": (dict(n_poses=3, n_points=90, seed=25, n_edges=255, **ALL), 3, 0),
    "e256": (dict(n_poses=3, n_points=90, seed=26, n_edges=256, stereo=0.5, **ALL), 3, 1),
    "e257": (dict(n_poses=3, n_points=90, seed=27, n_edges=257, stereo=1.0, **ALL), 3, 0),
    "gap": (dict(n_poses=6, n_points=40, seed=30, stereo=0.5, strip_pose=2, also_fixed=(4,)), 4, 1),
    "all_fixed": (dict(n_poses=3, n_points=20, seed=31, stereo=0.5, fix_all=True, **ALL), 4, 1),
    # a start 0.3 rad / 1 m off whose second iteration has two rejected trials before the accepted one
    "far": (dict(n_poses=4, n_points=30, seed=97, stereo=0.5, start_rot=0.3, start_t=1.0, start_pt=1.0), 6, 1),
}
SEAMS = ("init_f1", "f7", "f8", "f9", "f17")


def scene(name):
    return gs.scene(**FIXTURES[name][0])


@functools.lru_cache(maxsize=None)
def ref(name, n_iterations=None, stop_at=None):
    """the restatement's result of a fixture, computed once per session"""
    kw, it, robust = FIXTURES[name]
    return gr.run_scene(gs.scene(**kw), it if n_iterations is None else n_iterations, robust, stop_at)


def round_trip(T):
    return poseopt_ref.se3_to_T(poseopt_ref.se3_from_T(T)).astype(F32)


def deviation(T, X, r):
    """largest deviation of the float32 poses T (P, 4, 4) and points X (M, 3) from the restatement's in
    float32 ulps, a pose at its own scale, the points at the problem's"""
    dev = 0.0
    for a, b in zip(np.asarray(T).reshape(-1, 4, 4), r.Tcw):
        scale = max(1.0, float(np.abs(b).max()))
        dev = max(dev, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / (ULP * scale))
    if len(r.Xw):
        scale = max(1.0, float(np.abs(r.Xw).max()))
        dev = max(dev, float(np.abs(np.asarray(X).astype(np.float64) - r.Xw.astype(np.float64)).max()) / (ULP * scale))
    return dev


COUNTERS = ("iterations", "rejected", "stopped", "iterations_applied")


# ---------------------------------------------------------------- CPU: the restatement's own checks

@pytest.mark.parametrize("n", [6, NB - 6, NB, NB + 6, 2 * NB + 6])
def test_ref_blocked_order_solve(n):
    """against numpy.linalg.solve within test_ref_schur_solve_agrees_with_the_dense_solve's bound; the
    factor and y bit-equal to lm_ref.cholesky_solve's"""
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n))
    S = A @ A.T + np.eye(n)
    b = rng.standard_normal(n)
    x, L, y = gr.blocked_order_solve(S, b)
    x_dense = np.linalg.solve(S, b)
    rel = float(np.linalg.norm(x - x_dense) / np.linalg.norm(x_dense))
    bound = 2 * n * np.finfo(np.float64).eps * np.linalg.cond(S)
    print(f"n {n}: relative difference {rel:.3g}, bound {bound:.3g}")
    assert rel <= bound
    # lm_ref.cholesky_solve keeps L and y to itself: its loops, on the same inputs
    Lr = np.zeros((n, n))
    for j in range(n):
        s = float(S[j][j])
        for k in range(j):
            s -= Lr[j][k] * Lr[j][k]
        Lr[j][j] = np.sqrt(s)
        for i in range(j + 1, n):
            s = float(S[i][j])
            for k in range(j):
                s -= Lr[i][k] * Lr[j][k]
            Lr[i][j] = s / Lr[j][j]
    yr = np.zeros(n)
    for i in range(n):
        s = float(b[i])
        for k in range(i):
            s -= Lr[i][k] * yr[k]
        yr[i] = s / Lr[i][i]
    assert L.tobytes() == Lr.tobytes() and y.tobytes() == yr.tobytes()
    xr = np.array(lm_ref.cholesky_solve(S, b, 0.0))  # the row-ordered back-substitution: same x to rounding
    assert np.abs(x - xr).max() <= bound * np.abs(xr).max()
    S[n // 2, n // 2] = -1.0
    assert gr.blocked_order_solve(S, b) is None and lm_ref.cholesky_solve(S, b, 0.0) is None


def test_ref_noise_free_stereo_scene_recovers_the_truth():
    """noise-free observations with stereo ones among them (no gauge is free: pose 0 is fixed and the
    right coordinates give the scale): poses to 1e-5 and points to 1e-4 m, test_localba.py's bounds with
    the same derivation (the float32 rounding of the observations over the narrowest triangulation
    angle, times ten)"""
    s = gs.scene(n_poses=7, n_points=60, seed=91, noise=0.0, stereo=0.3, see=1.0)
    r = gr.run_scene(s, 20, 0)
    pose_err = float(np.abs(r.Tcw.astype(np.float64) - s["Tcw_true"]).max())
    point_err = float(np.abs(r.Xw.astype(np.float64) - s["Xw_true"]).max())
    start = float(np.abs(s["Tcw"].astype(np.float64) - s["Tcw_true"]).max())
    print(f"pose error {pose_err:.2e} (start {start:.2e}), point error {point_err:.2e}, iterations {r.iterations}")
    assert (s["obs"][:, 2] >= 0).any() and start > 1e-2 and pose_err < 1e-5 and point_err < 1e-4


def test_ref_every_accepted_trial_lowers_the_robust_chi2():
    s = gs.scene(n_poses=5, n_points=50, seed=92, start_rot=0.1, start_t=0.3, start_pt=0.3)
    assert (s["obs"][:, 2] < 0).all()  # monocular only
    tr = gr.run_scene(s, 10, 1).trace
    chi = tr.first_chi
    assert any(tr.trials) and len(tr.trials) == len(tr.chi_after)
    for accepted, after in zip(tr.trials, tr.chi_after):
        assert (after < chi) if accepted else (after == chi)
        chi = after


def test_ref_the_monocular_delta_is_5_99():
    assert gr.DELTA_MONO != poseopt_ref.DELTA_MONO and gr.DELTA_MONO == float(F32(np.sqrt(5.99)))
    assert gr.DSQR_MONO == float(F32(gr.DELTA_MONO * gr.DELTA_MONO))
    kw, it, robust = FIXTURES["init_f1"]

    def localba_deltas(job):
        job.delta = np.where(job.stereo, poseopt_ref.DELTA_STEREO, poseopt_ref.DELTA_MONO)
        job.dsqr = np.where(job.stereo, poseopt_ref.DSQR_STEREO, poseopt_ref.DSQR_MONO)

    a, b = ref("init_f1"), gr.run_scene(gs.scene(**kw), it, robust, job_hook=localba_deltas)
    assert a.Tcw.tobytes() != b.Tcw.tobytes() or a.Xw.tobytes() != b.Xw.tobytes()


def test_ref_active_set_and_round_trips():
    """a pose without edges and a point without edges keep the round trip; all poses fixed optimises the
    points alone; n_iterations = 0 and E = 0 write the round trip"""
    s, r = scene("gap"), ref("gap")
    assert not s["fixed"][2] and (s["pose_idx"] != 2).all() and s["fixed"][[0, 4]].all()
    assert r.n_free == 3 and r.iterations >= 1
    for p in (0, 2, 4):
        assert r.Tcw[p].tobytes() == round_trip(s["Tcw"][p]).tobytes()
    for p in (1, 3, 5):
        assert r.Tcw[p].tobytes() != round_trip(s["Tcw"][p]).tobytes()
    s, r = scene("e63"), ref("e63")
    seen = np.zeros(len(s["Xw"]), bool)
    seen[s["point_idx"]] = True
    assert 0 < seen.sum() < len(seen) and r.n_active_points == seen.sum()
    assert r.Xw[~seen].tobytes() == s["Xw"][~seen].tobytes() and (r.Xw[seen] != s["Xw"][seen]).any()
    s, r = scene("all_fixed"), ref("all_fixed")
    assert r.n_free == 0 and r.iterations >= 1 and r.n_active_points == len(s["Xw"])
    assert all(r.Tcw[p].tobytes() == round_trip(s["Tcw"][p]).tobytes() for p in range(len(s["Tcw"])))
    assert (r.Xw != s["Xw"]).any()
    for name, r in (("e0", ref("e0")), ("m0", ref("m0")), ("f7", ref("f7", 0))):
        s = scene(name)
        assert r.iterations == 0 and r.iterations_applied == 0 and r.stopped == 0 and r.trace.polls == 0
        assert all(r.Tcw[p].tobytes() == round_trip(s["Tcw"][p]).tobytes() for p in range(len(s["Tcw"])))
        assert r.Xw.tobytes() == s["Xw"].tobytes()
    s = scene("f7")  # a fixed pose does not in general keep its bits
    assert any(round_trip(s["Tcw"][p]).tobytes() != s["Tcw"][p].tobytes() for p in range(len(s["Tcw"])))


def test_ref_stop_at_either_poll_equals_a_shorter_flagless_run():
    full = ref("far")
    tr = full.trace
    assert any(not a and k + 1 < len(tr.trials) for k, a in enumerate(tr.trials)) and full.rejected >= 1
    seen = set()
    for k in range(tr.polls + 1):
        a = ref("far", None, k)
        b = ref("far", a.iterations_applied)
        seen.add(a.stopped)
        assert a.stopped in ((1, 2) if k < tr.polls else (0,))
        assert a.iterations_applied == a.iterations - (1 if a.stopped == 2 else 0)
        assert a.Tcw.tobytes() == b.Tcw.tobytes() and a.Xw.tobytes() == b.Xw.tobytes(), k
    assert seen == {0, 1, 2}
    assert ref("far", None, 0).iterations == 0


def permuted(name, k):
    kw, it, robust = FIXTURES[name]
    s = gs.scene(**kw)
    return gr.run_scene(s, it, robust, None, np.random.default_rng(1000 + k).permutation(len(s["Xw"])), 2000 + k)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_ref_permutation_spread_of_every_fixture(name):
    """the same scene with its points permuted and its edges permuted within each point (every sum
    rounds differently), 8 times: every run is decisive, the integer outcomes are equal, and poses and
    points stay within the measured worst the GPU bound is made from"""
    a = ref(name)
    assert gr.decisive(a), (name, min(a.trace.margins))
    worst = 0.0
    for k in range(PERMUTATIONS):
        b = permuted(name, k)
        assert gr.decisive(b), (name, k, min(b.trace.margins))
        assert all(getattr(a, c) == getattr(b, c) for c in COUNTERS + ("n_free", "n_active_points")), (name, k)
        worst = max(worst, deviation(b.Tcw, b.Xw, a))
    print(f"{name}: permutation spread {worst:.3f} ulp, iterations {a.iterations}, rejected {a.rejected}")
    assert worst <= MEASURED_WORST + 1e-3


def test_scene_preconditions():
    """what the named fixtures are for holds"""
    assert [ref(n).n_free for n in SEAMS] == [1, NB // 6 - 1, NB // 6, NB // 6 + 1, 2 * NB // 6 + 1]
    s, r = scene("init_f1"), ref("init_f1")
    assert len(s["Tcw"]) == 2 and len(s["Xw"]) == 150 and (s["obs"][:, 2] < 0).all() and FIXTURES["init_f1"][1:] == (20, 1)
    s = scene("p70")
    assert len(s["Tcw"]) == 70 and (s["point_idx"] == 0).sum() == 70 > 64 and (s["pose_idx"] == 1).sum() > 256
    assert ref("p70").n_free == 69
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        assert len(scene(f"m{n}")["Xw"]) == n and len(scene(f"e{n}")["obs"]) == n
    assert ref("e1").n_free == 0 and ref("e1").n_active_points == 1
    kinds = set()
    for name, (kw, it, robust) in FIXTURES.items():
        st = scene(name)["obs"][:, 2] >= 0
        if len(st):
            kinds.add(("mono", "mixed", "stereo")[int(st.any()) + int(st.all())] + str(robust))
    assert kinds == {a + b for a in ("mono", "mixed", "stereo") for b in "01"}


# ---------------------------------------------------------------- CPU: argument checks of the library

ARRAYS = tuple(n for n, *_ in globalba.INPUTS) + tuple(n for n, *_ in globalba.OUTPUTS)


def _args(form, **kw):
    """the library call with fake non-null pointers (never dereferenced by a rejected call) and real edge
    indices for the host form's checks"""
    a = dict(P=3, M=4, E=6, it=5, robust=1, stop=None, res=1 << 20, ws=1 << 30, ws_bytes=1 << 40)
    a.update({name: 1 << (21 + k) for k, name in enumerate(ARRAYS)})
    a["edge_pose"] = np.array([0, 1, 2, 0, 1, 2], np.int32)
    a["edge_point"] = np.array([0, 0, 1, 2, 3, 3], np.int32)
    a.update(kw)
    ptr = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    arr = [ptr(a[n]) if form == "host" or a[n] is None else 1 << 23 for n in ARRAYS]
    L = globalba._lib()
    fn = L.orbgpu_bundle_adjustment if form == "host" else L.orbgpu_bundle_adjustment_device
    tail = () if form == "host" else (None,)
    return fn(a["P"], a["M"], a["E"], *arr[:8], a["it"], a["robust"], a["stop"], *arr[8:], a["res"], a["ws"],
              a["ws_bytes"], *tail)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_checks_need_no_device(form):
    """rejected on the host before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    for name in ("P", "M", "E", "it"):
        assert _args(form, **{name: -1}) == E, name
    for name in (*ARRAYS, "res"):
        assert _args(form, **{name: None}) == E, name
        assert "null" in orbgpu.last_error(), name
    need = globalba.workspace_bytes(3, 4, 6)
    assert need > 0 and need % 8 == 0
    assert _args(form, ws_bytes=need - 1) == E and "workspace" in orbgpu.last_error()
    assert _args(form, ws=(1 << 30) + 4) == E
    if form == "device":
        assert _args(form, ws=None) == E
    assert globalba.workspace_bytes(-1, 0, 0) == 0 and globalba.workspace_bytes(0, -1, 0) == 0
    assert globalba.workspace_bytes(0, 0, -1) == 0
    assert globalba.workspace_bytes(2 ** 31 - 1, 1, 1) == 0  # (6 P)^2 doubles do not fit a size_t
    assert globalba.workspace_bytes(4, 4, 6) > need > globalba.workspace_bytes(3, 4, 5)
    # the dense reduced system: (6 P + 1) 6 P doubles
    assert globalba.workspace_bytes(300, 0, 0) - globalba.workspace_bytes(299, 0, 0) > 8 * 6 * 6 * 599


def test_edge_index_checks_of_the_host_form_need_no_device():
    E = orbgpu.ERR_ARG
    for k, v in ((2, 3), (2, -1), (5, 7)):
        ep = np.array([0, 1, 2, 0, 1, 2], np.int32)
        ep[k] = v
        assert _args("host", edge_pose=ep) == E and "out of range" in orbgpu.last_error(), (k, v)
    for k, v in ((5, 4), (0, -1)):
        el = np.array([0, 0, 1, 2, 3, 3], np.int32)
        el[k] = v
        assert _args("host", edge_point=el) == E and "out of range" in orbgpu.last_error(), (k, v)
    el = np.array([0, 0, 1, 0, 3, 3], np.int32)
    assert _args("host", edge_point=el) == E and "decrease" in orbgpu.last_error()


def _header_struct(name):
    """(size, {member: offset}) of a struct of include/orbgpu_globalba.h, from its text"""
    text = (ROOT / "include" / "orbgpu_globalba.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, offsets = 0, {}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        size = {"int": 4, "double": 8}[ctype]
        for member in rest.split(","):
            off = (off + size - 1) // size * size
            offsets[member.strip()] = off
            off += size
    return off, offsets


def test_python_wrapper_and_struct_layout():
    """sizes and offsets agree between ctypes, the numpy dtype and the header"""
    hsize, hoff = _header_struct("orbgpu_ba_result")
    assert ctypes.sizeof(globalba.BAResult) == globalba.RESULT_DTYPE.itemsize == hsize == 56
    assert [f[0] for f in globalba.BAResult._fields_] == list(globalba.RESULT_DTYPE.names) == list(hoff)
    for field in globalba.RESULT_DTYPE.names:
        assert getattr(globalba.BAResult, field).offset == globalba.RESULT_DTYPE.fields[field][1] == hoff[field], field
    s = scene("f7")
    with pytest.raises(ValueError):
        globalba.pack(s["Tcw"], s["fixed"][:-1], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"], s["obs"], s["inv_sigma2"])


@pytest.fixture(scope="module")
def globalba_args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("globalba_args") / "globalba_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "globalba_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(globalba_args_main):
    """argument checks, the edge index checks of the host form and the workspace layout, compiled for the
    host with -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(globalba_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
    r = subprocess.run([str(globalba_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = {k: int(v) for k, v in re.findall(r"(\S+) (\d+)", r.stdout)}
    R = globalba.BAResult
    assert got == {"orbgpu_ba_result": ctypes.sizeof(R), "result.n_free": R.n_free.offset,
                   "result.first_chi2": R.first_chi2.offset, "result.last_lambda": R.last_lambda.offset}


# ---------------------------------------------------------------- the C++ adapter

@pytest.fixture(scope="module")
def globalba_main(tmp_path_factory):
    """tests/cpp/globalba_main.cpp against BundleAdjuster.h and the cvlite stand-ins, one g++ line"""
    pkg = ROOT / "orb-slam2-annotation_amd"
    exe = tmp_path_factory.mktemp("globalba") / "globalba_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'tests' / 'cpp'}", '-DORBGPU_CV_HEADER="cvlite.hpp"', "-pthread", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "globalba_main.cpp"), f"-L{pkg}", "-lorbgpu", f"-Wl,-rpath,{pkg}"],
                   check=True)
    return exe


TABLE = (1.0 / 1.2 ** (2.0 * np.arange(8))).astype(F32)


def _adapter_world(s, rng, n_iterations, robust, n_loop_kf, through_map, stop=-1.0, only_bad=False):
    """Stand-in keyframes and MapPoints around a scene, with what the gather must skip interleaved: a bad
    keyframe and a keyframe that is not listed and whose mnId is above every listed one (both observe
    points), a bad MapPoint and a MapPoint only those two keyframes observe (not included: not written
    back).  Keyframe and MapPoint indices are shuffled, so neither vpKFs, vpMP nor GetObservations()
    (ordered by keyframe index) is in the scene's order.  Returns (blob for globalba_main, the problem as
    the gather must produce it, the keyframe index of each of its poses, the MapPoint index of each of its
    points, the MapPoints that are written back)."""
    P, M = len(s["Tcw"]), len(s["Xw"])
    n_kf, n_mp = P + 2, M + 2
    kf_of_pose = rng.permutation(n_kf)[:P]
    bad_kf, late_kf = sorted(set(range(n_kf)) - set(kf_of_pose.tolist()))
    mp_of_point = rng.permutation(n_mp)[:M]
    bad_mp, lone_mp = sorted(set(range(n_mp)) - set(mp_of_point.tolist()))
    octave = np.rint(np.log(1.0 / s["inv_sigma2"].astype(np.float64)) / (2 * np.log(1.2))).astype(int)
    assert np.array_equal(TABLE[octave], s["inv_sigma2"])
    keys = [[] for _ in range(n_kf)]      # per keyframe: (x, y, octave, uRight)
    obs_of = [[] for _ in range(n_mp)]    # per MapPoint: (keyframe, keypoint)
    for e in range(len(s["obs"])):
        k, m = int(kf_of_pose[s["pose_idx"][e]]), int(mp_of_point[s["point_idx"][e]])
        keys[k].append((*s["obs"][e][:2], octave[e], s["obs"][e][2]))
        obs_of[m].append((k, len(keys[k]) - 1))
    for k in (bad_kf, late_kf):           # no edge comes from these
        for m in [int(v) for v in mp_of_point[:3]] + [lone_mp, bad_mp]:
            keys[k].append((11.0, 12.0, 0, -1.0))
            obs_of[m].append((k, len(keys[k]) - 1))
    ids = np.zeros(n_kf, int)
    order = rng.permutation(P)
    for rank, p in enumerate(order):      # pose 0 is keyframe 0; the others get distinct ids in any order
        ids[kf_of_pose[p]] = 0 if p == 0 else 2 * rank + 3
    ids[kf_of_pose[0]] = 0
    ids[bad_kf], ids[late_kf] = 1, ids.max() + 5
    blob = [n_kf, n_mp, n_iterations, stop, n_loop_kf, robust, float(through_map), 0.0, *TABLE]
    for k in range(n_kf):
        pose = np.nonzero(kf_of_pose == k)[0]
        T = s["Tcw"][pose[0]][:3].reshape(-1) if len(pose) else np.eye(4, dtype=F32)[:3].reshape(-1)
        cam = s["cam"][pose[0]] if len(pose) else s["cam"][0]
        bad = k == bad_kf or (only_bad and k != late_kf)
        blob += [ids[k], float(bad), float(k != late_kf), *cam, *T, len(keys[k])]
        for row in keys[k]:
            blob += list(row)
    for m in range(n_mp):
        point = np.nonzero(mp_of_point == m)[0]
        X = s["Xw"][point[0]] if len(point) else (9.0, 9.0, 9.0)
        blob += [100 + m, float(m == bad_mp or only_bad), *X, len(obs_of[m])]
        for row in obs_of[m]:
            blob += list(row)
    # what the gather produces: the listed keyframes that are not bad in index order, the MapPoints that
    # are not bad in index order (the lone one included, without an edge), edges by point and inside by
    # keyframe index
    pose_kfs = sorted(int(k) for k in kf_of_pose)
    pose_of_kf = {k: i for i, k in enumerate(pose_kfs)}
    scene_pose = [int(np.nonzero(kf_of_pose == k)[0][0]) for k in pose_kfs]
    point_mps = sorted([int(m) for m in mp_of_point] + [lone_mp])
    ep, el, ob, w = [], [], [], []
    for i, m in enumerate(point_mps):
        for k, idx in sorted(obs_of[m]):
            if k in pose_of_kf:
                row = keys[k][idx]
                ep.append(pose_of_kf[k]), el.append(i)
                ob.append((row[0], row[1], row[3])), w.append(TABLE[int(row[2])])
    Xw = np.stack([s["Xw"][np.nonzero(mp_of_point == m)[0][0]] if m != lone_mp else F32([9, 9, 9]) for m in point_mps])
    fixed = np.array([1 if ids[k] == 0 else 0 for k in pose_kfs], np.uint8)  # mnId == 0 alone, whatever the scene says
    problem = dict(Tcw=s["Tcw"][scene_pose], fixed=fixed, cam=s["cam"][scene_pose], Xw=Xw,
                   pose_idx=np.array(ep, np.int32), point_idx=np.array(el, np.int32), obs=np.array(ob, F32).reshape(-1, 3),
                   inv_sigma2=np.array(w, F32))
    written = [m for m in point_mps if m != lone_mp]
    return np.array(blob, np.float64), problem, pose_kfs, point_mps, written


def _run_adapter(exe, tmp_path, blob):
    (tmp_path / "scene.bin").write_bytes(np.asarray(blob, np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path / "scene.bin"), str(tmp_path / "out.txt")], check=True, timeout=120)
    return [line.split() for line in (tmp_path / "out.txt").read_text().split("\n") if line]


def test_adapter_builds_and_with_nothing_that_is_not_bad_touches_nothing(globalba_main, tmp_path):
    """BundleAdjuster.h compiles against the stand-ins with -Wall -Wextra -Werror; when every keyframe and
    MapPoint is bad there is no vertex: no device is needed and nothing is written"""
    blob, *_ = _adapter_world(scene("f7"), np.random.default_rng(5), 4, 1, 0, 1, only_bad=True)
    lines = _run_adapter(globalba_main, tmp_path, blob)
    assert {l[0] for l in lines} == {"G", "g"} and all(l[2] == "0" and len(l) == 3 for l in lines)


# ---------------------------------------------------------------- GPU

def _torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


G = 64  # guard bytes around every device array


def _guarded(torch, a, fill=None):
    """a device copy of `a` (or `fill` bytes in its shape) between two runs of G guard bytes"""
    host = np.array(a, order="C")  # a writable copy: torch.from_numpy takes no read-only array
    nbytes = host.nbytes
    pad = (-nbytes) % 8
    full = torch.full((G + nbytes + pad + G,), 0xC3, dtype=torch.uint8, device="cuda")
    if fill is None:
        if nbytes:
            full[G:G + nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8)).cuda()
    else:
        full[G:G + nbytes] = fill
    view = full[G:G + nbytes].view(torch.from_numpy(host[:0]).dtype).reshape(host.shape)
    return full, view, nbytes


def _guards_intact(bufs):
    for full, _, nbytes in bufs:
        h = full.cpu().numpy()
        assert (h[:G] == 0xC3).all() and (h[G + nbytes:] == 0xC3).all()


def run_device(s, n_iterations, robust, stream=None, stop=None, workspace=None, mutate=None, before_call=None):
    """the device form on guarded copies, outputs and workspace pre-filled with 0x5A; returns (record,
    Tcw_out (P, 16), Xw_out (M, 3), workspace tensor triple); checks the guards and that no input changed"""
    torch = _torch_gpu()
    a = globalba.pack(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"], s["obs"], s["inv_sigma2"])
    if mutate:
        mutate(a)
    tp, tm, te = len(a["Tcw"]), len(a["Xw"]), len(a["obs"])
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d_in = [_guarded(torch, a[n]) for n, *_ in globalba.INPUTS]
        d_T = _guarded(torch, np.zeros((tp, 16), F32), 0x5A)
        d_X = _guarded(torch, np.zeros((tm, 3), F32), 0x5A)
        ws = workspace or _guarded(torch, np.zeros(globalba.workspace_bytes(tp, tm, te), np.uint8), 0x5A)
        before = [f.clone() for f, *_ in d_in]
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    if before_call:
        before_call()
    res = globalba.bundle_adjustment_device(*(v for _, v, _ in d_in), n_iterations, robust, d_T[1], d_X[1], ws[1],
                                            stream=stream, stop=stop)
    torch.cuda.synchronize()
    for (f, *_), b in zip(d_in, before):
        assert torch.equal(f, b)
    _guards_intact(d_in + [d_T, d_X, ws])
    return res, d_T[1].cpu().numpy(), d_X[1].cpu().numpy(), ws


def check_against_ref(res, T, X, r, label):
    assert gr.decisive(r), label  # the condition on the inputs
    dev = deviation(T, X, r)
    print(f"{label}: deviation {dev:.3f} ulp (bound {ULP_BOUND:.3f}), iterations {res['iterations']} rejected "
          f"{res['rejected']} stopped {res['stopped']} applied {res['iterations_applied']}, n_free {res['n_free']}; "
          f"restatement {r.iterations} {r.rejected} {r.stopped} {r.iterations_applied}; chi2 {res['first_chi2']:.6g} -> "
          f"{res['last_chi2']:.6g} ({r.first_chi:.6g} -> {r.last_chi:.6g})")
    assert res["status"] == 0 and T.shape == (len(r.Tcw), 16) and X.shape == r.Xw.shape
    assert (int(res["n_free"]), int(res["n_active_points"])) == (r.n_free, r.n_active_points), label
    assert tuple(int(res[c]) for c in COUNTERS) == tuple(getattr(r, c) for c in COUNTERS), label
    assert dev <= ULP_BOUND, (label, dev)
    assert np.array_equal(T[:, 12:], np.tile(F32([0, 0, 0, 1]), (len(T), 1))), label
    # sums of up to 2^15 terms associated differently: 2^15 eps = 4e-12 of a chi2; lambda follows rho, whose
    # numerator is a difference of two chi2 at least 1e-6 of them (decisive): 4e-6 of lambda
    for got, want, tol in ((res["first_chi2"], r.first_chi, 1e-9), (res["last_chi2"], r.last_chi, 1e-9),
                           (res["last_lambda"], r.last_lambda, 1e-4)):
        assert abs(got - want) <= tol * abs(want), label
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_gpu_fixture(name):
    """every fixture through the device form; the host form gives the same bytes"""
    kw, it, robust = FIXTURES[name]
    s, r = scene(name), ref(name)
    res, T, X, _ = run_device(s, it, robust)
    check_against_ref(res, T, X, r, name)
    T1, X1, res1 = globalba.bundle_adjustment(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"],
                                              s["obs"], s["inv_sigma2"], it, robust)
    assert T1.tobytes() == T.tobytes() and X1.tobytes() == X.tobytes() and res1.tobytes() == res.tobytes()


@pytest.mark.gpu
def test_gpu_zero_iterations_write_the_round_trip():
    s, r = scene("f7"), ref("f7", 0)
    res, T, X, _ = run_device(s, 0, 1)
    assert T.tobytes() == r.Tcw.tobytes() and X.tobytes() == s["Xw"].tobytes()
    assert tuple(int(res[c]) for c in COUNTERS) == (0, 0, 0, 0) and res["n_free"] == r.n_free


@pytest.mark.gpu
def test_gpu_determinism_and_a_used_workspace():
    """two calls give equal bytes, the second on the workspace the first left"""
    kw, it, robust = FIXTURES["f17"]
    s = scene("f17")
    res, T, X, ws = run_device(s, it, robust)
    res2, T2, X2, _ = run_device(s, it, robust, workspace=ws)
    assert res.tobytes() == res2.tobytes() and T.tobytes() == T2.tobytes() and X.tobytes() == X2.tobytes()
    kw, it, robust = FIXTURES["far"]
    res3, T3, X3, _ = run_device(scene("far"), it, robust)
    res4, T4, X4, _ = run_device(scene("far"), it, robust)
    assert res3.tobytes() == res4.tobytes() and T3.tobytes() == T4.tobytes() and X3.tobytes() == X4.tobytes()


@pytest.mark.gpu
def test_gpu_device_form_on_a_stream():
    torch = _torch_gpu()
    kw, it, robust = FIXTURES["f9"]
    res, T, X, _ = run_device(scene("f9"), it, robust, stream=torch.cuda.Stream())
    check_against_ref(res, T, X, ref("f9"), "f9 on a stream")


@pytest.mark.gpu
def test_gpu_nan_pose_ends_inside_the_loop_bound():
    """a NaN in a free pose: every trial is rejected, the call returns within n_iterations (1 + 10)
    passes, and the other vertices keep their round trip"""
    kw, it, robust = FIXTURES["f7"]
    s = gs.scene(nan_pose=1, **kw)
    res, T, X, _ = run_device(s, it, robust)
    trials = int(res["rejected"])
    print(f"NaN pose: iterations {res['iterations']}, rejected {trials}")
    assert res["status"] == 0 and 1 <= res["iterations"] <= it and res["iterations"] <= trials <= 10 * it
    for p in range(len(s["Tcw"])):
        if p != 1:
            assert T[p].tobytes() == round_trip(s["Tcw"][p]).tobytes(), p
    assert X.tobytes() == s["Xw"].tobytes()


@pytest.mark.gpu
def test_gpu_bad_index_is_rejected_and_nothing_is_written():
    s = scene("e65")
    for key, at, value in (("edge_pose", 40, len(s["Tcw"])), ("edge_pose", 0, -1), ("edge_point", 64, len(s["Xw"])),
                           ("edge_point", 30, 0)):
        def mutate(a, key=key, at=at, value=value):
            a[key] = a[key].copy()
            a[key][at] = value
        res, T, X, _ = run_device(s, 3, 1, mutate=mutate)
        assert res["status"] == -1 and res["iterations"] == 0, (key, at)
        assert (T.view(np.uint8) == 0x5A).all() and (X.view(np.uint8) == 0x5A).all(), (key, at)


@pytest.mark.gpu
def test_gpu_stop_flag():
    """preset: no iteration begins and the round trip is written.  Set from a second host thread at an
    arbitrary moment of a 20-iteration run: whatever stopped and iterations_applied come back, the
    outputs are byte-equal to a flagless call with n_iterations = iterations_applied"""
    kw, it, robust = FIXTURES["init_f1"]
    s = scene("init_f1")
    res, T, X, _ = run_device(s, it, robust, stop=globalba.StopFlag(True))
    assert (int(res["iterations"]), int(res["stopped"]), int(res["iterations_applied"])) == (0, 1, 0)
    assert T.tobytes() == ref("init_f1", 0).Tcw.tobytes() and X.tobytes() == s["Xw"].tobytes()
    seen = []
    for spin in (0, 2000, 8000, 30000, 120000):  # no sleep: the second thread counts, then sets the flag
        flag, go = globalba.StopFlag(), threading.Event()
        t = threading.Thread(target=lambda: (go.wait(), sum(range(spin)), flag.set()))
        t.start()  # it waits for the call to begin, which releases the interpreter lock to it
        res, T, X, _ = run_device(s, it, robust, stop=flag, before_call=go.set)
        t.join()
        seen.append((int(res["stopped"]), int(res["iterations"]), int(res["iterations_applied"])))
        assert res["stopped"] in (0, 1, 2)
        assert res["iterations_applied"] == res["iterations"] - (1 if res["stopped"] == 2 else 0)
        res2, T2, X2, _ = run_device(s, int(res["iterations_applied"]), robust)
        assert res2["stopped"] == 0 and T.tobytes() == T2.tobytes() and X.tobytes() == X2.tobytes(), seen
    print(f"stop flag from a second thread: (stopped, iterations, applied) {seen}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_loop_kf,through_map", [("f9", 0, 1), ("gap", 7, 0)])
def test_gpu_adapter(globalba_main, tmp_path, name, n_loop_kf, through_map):
    """BundleAdjustmentGPU / GlobalBundleAdjustemntGPU on stand-in keyframes with a bad keyframe, a keyframe
    above maxKFid, a bad MapPoint and a MapPoint left without an edge interleaved: every SetPose and
    SetWorldPos value and the call order (nLoopKF == 0), or mTcwGBA, mPosGBA and mnBAGlobalForKF,
    against the restatement run on what the gather must produce"""
    _torch_gpu()
    kw, it, robust = FIXTURES[name]
    blob, problem, pose_kfs, point_mps, written = _adapter_world(scene(name), np.random.default_rng(3), it, robust,
                                                                 n_loop_kf, through_map, stop=0.0)
    r = gr.run_scene(problem, it, robust)
    assert gr.decisive(r) and r.iterations >= 1
    lines = _run_adapter(globalba_main, tmp_path, blob)
    hexf = lambda words: np.array([int(w, 16) for w in words], np.uint32).view(F32)
    calls = [l for l in lines if l[0] not in "Gg"]
    G = {int(l[1]): l[2:] for l in lines if l[0] == "G"}
    g = {int(l[1]): l[2:] for l in lines if l[0] == "g"}
    assert len(G) == len(pose_kfs) + 2 and len(g) == len(point_mps) + 1
    if n_loop_kf == 0:
        assert [l[0] for l in calls] == ["P"] * len(pose_kfs) + ["W", "U"] * len(written)
        NP = len(pose_kfs)
        assert [int(l[1]) for l in calls[:NP]] == pose_kfs
        assert [int(l[1]) for l in calls[NP::2]] == written == [int(l[1]) for l in calls[NP + 1::2]]
        T = np.stack([hexf(l[2:]) for l in calls[:NP]])
        X = np.stack([hexf(l[2:]) for l in calls[NP::2]])
        assert all(v == ["0"] for v in G.values()) and all(v == ["0"] for v in g.values())
    else:
        assert calls == []
        for k, v in G.items():
            assert v[0] == (str(n_loop_kf) if k in pose_kfs else "0") and len(v) == (17 if k in pose_kfs else 1), k
        for m, v in g.items():
            assert v[0] == (str(n_loop_kf) if m in written else "0") and len(v) == (4 if m in written else 1), m
        T = np.stack([hexf(G[k][1:]) for k in pose_kfs])
        X = np.stack([hexf(g[m][1:]) for m in written])
    keep = [i for i, m in enumerate(point_mps) if m in written]
    full = r.Xw.copy()
    full[keep] = X
    dev = deviation(T, full, r)
    print(f"adapter {name}: deviation {dev:.3f} ulp, iterations {r.iterations}")
    assert dev <= ULP_BOUND
