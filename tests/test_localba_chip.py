"""Local bundle adjustment of one neighbourhood over the whole chip
(include/orbgpu_localba_chip.h, csrc/localba_chip.hip, csrc/ba_phases.h) against
the numpy restatement tests/localba_chip_ref.py: localba_ref's two rounds on
globalba_ref's solver, with g2o's polls of the stop flag.

The scenes are test_localba.py's SIZES and CASES and five of this file's: f7 /
f8 / f9 (7, 8 and 9 free local poses: 42, 48 and 54 unknowns around the
Cholesky panel of 48), wide_pose (local poses with 270 edges each: a pose's list
crosses a workgroup) and far_both, a start 0.6 rad / 2 m off whose trace has
rejected trials that another follows in BOTH rounds, so that every kind of poll
occurs (test_localba.py's `far` rejects in the second round only).

Decisions.  The GPU tests compare the LM counters for equality, so every chi2
decision of the restatement (accept / reject, rho == 0, the stop criterion)
must be decisive by globalba_ref.decisive's rule: 1e-6 relative from its
threshold, under the identity and 8 permutations.  With LocalMapping's 5 + 10
iterations that cannot hold on a scene that converges: its last trials change
chi2 by 1e-7 .. 1e-15 of it, and whether such a trial is accepted is rounding
noise (test_localba.py compares the counters "in range only" for that reason).
ITERATIONS below therefore gives 9 of test_localba.py's 22 scenes the largest
iteration limits (searched on the CPU downwards from 5 and 10) at which every
decision is decisive under all 9 orders; the other 18 fixtures run 5 + 10.  The
9 also run 5 + 10 on the GPU, with everything compared but the four LM
counters, which are then in range only.

Bound.  MEASURED_WORST is the restatement's largest float32 deviation under the
8 permutations, measured on the CPU: 0.0625 ulp on far_both (15 iterations from
2 m off have not converged, and the start's sensitivity shows), 0.000 on every
other fixture; ULP_BOUND = max(2, 4 x MEASURED_WORST) = 2 ulp.
test_ref_margins_and_permutation_spread asserts the measurement.

Against localba_ref (the back-substitution order is the one difference in
arithmetic) at 5 + 10 iterations: erase, flag_first, n_bad_first and n_erase
equal and 0.000 ulp on all 27 fixtures, measured on the CPU.

Measured on an MI355X against the restatement: 0.000 ulp on all 27 fixtures at
their decisive limits and on the 9 at 5 + 10, every counter equal (at 5 + 10
the LM counters too, as it happened), at a stop of each kind of poll, through
the C++ adapter and through the map-mirror chain.
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
import localba
import localba_chip_ref as cr
import localba_ref
import orbgpu
from test_localba import CASES, SIZES, bound_of as localba_bound_of, deviation, scene

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
MARGIN = 1e-6
PERMUTATIONS = 8
NB = 48  # csrc/chol_blocked.h: the panel width of the blocked Cholesky
MEASURED_WORST = 0.0625
ULP_BOUND = max(2.0, 4.0 * MEASURED_WORST)

NEW = {
    "f7": dict(n_local=7, n_fixed=2, n_points=60, seed=770, stereo=0.4),
    "f8": dict(n_local=8, n_fixed=2, n_points=60, seed=780, stereo=0.4),
    "f9": dict(n_local=9, n_fixed=2, n_points=60, seed=790, stereo=0.4),
    "wide_pose": dict(n_local=2, n_fixed=1, n_points=270, seed=900, stereo=0.3, see=1.0),
    "far_both": dict(n_local=3, n_fixed=2, n_points=40, seed=6, stereo=0.5, noise=0.5, start_rot=0.6, start_t=2.0,
                     start_pt=2.0),
}
FIXTURES = {**SIZES, **CASES, **NEW}
FULL = (5, 10)  # Optimizer.cpp:760, 813
# the largest limits at which every decision is decisive under the identity and 8 permutations (see above)
ITERATIONS = {"p2": (5, 1), "p16_e64": (5, 3), "e65": (3, 3), "p64_e256": (4, 3), "all_fixed": (5, 2), "far": (3, 4),
              "clean": (4, 4), "all_flagged_pose": (5, 5), "single": (3, 4)}
THREAD_LIMITS = (8, 12)  # far_both with room for a flag set while it runs; decisive (asserted)


def limits(name):
    return ITERATIONS.get(name, FULL)


def bound_of(name):
    return max(ULP_BOUND, localba_bound_of(name))


@functools.lru_cache(maxsize=None)
def ref(name, iterations=None, stop_at=None):
    """the restatement's result of a fixture, computed once per session and left unchanged"""
    return cr.run_scene(scene(**FIXTURES[name]), limits(name) if iterations is None else iterations, stop_at)


def permuted(name, k):
    s = scene(**FIXTURES[name])
    return cr.run_scene(s, limits(name), None, np.random.default_rng(1000 + k).permutation(len(s["Xw"])), 2000 + k)


def check_margins(r, s, what):
    m_chi, m_z = cr.margins(r, s["obs"])
    assert m_chi >= MARGIN and m_z >= MARGIN, (what, m_chi, m_z)
    assert cr.decisive(r), (what, min(m for tr in r.trace for m in tr.margins))


COUNTERS = ("lm_iterations", "lm_rejected", "stopped", "iterations_applied")
SETS = ("n_free", "n_active_points")
SCALARS = ("rounds", "n_bad_first", "n_erase", "polls", "stop_poll")


def counters(r):
    return tuple(tuple(int(v) for v in getattr(r, c)) for c in COUNTERS + SETS) + tuple(int(getattr(r, c)) for c in SCALARS)


# ---------------------------------------------------------------- CPU: the restatement

@pytest.mark.parametrize("name", list(FIXTURES))
def test_ref_margins_and_permutation_spread(name):
    """the identity and 8 permutations of the point order and of the edge order within points: every chi2
    either check reads is 1e-6 (relative) from its threshold, every depth 1e-6 from 0, every LM decision
    decisive; then the integer outcomes are equal and poses and points within the measured worst"""
    s, a = scene(**FIXTURES[name]), ref(name)
    check_margins(a, s, name)
    runs = [permuted(name, k) for k in range(PERMUTATIONS)]
    for k, b in enumerate(runs):
        check_margins(b, s, (name, k))
    worst = 0.0
    for k, b in enumerate(runs):
        assert counters(a) == counters(b) and a.poll_kinds == b.poll_kinds, (name, k)
        assert np.array_equal(a.erase, b.erase) and np.array_equal(a.flag_first, b.flag_first), (name, k)
        worst = max(worst, deviation(b.Tcw, b.Xw, a))
    print(f"{name}: permutation spread {worst:.4f} ulp at {limits(name)}, iterations {a.lm_iterations}, rejected "
          f"{a.lm_rejected}, polls {a.polls}")
    assert worst <= MEASURED_WORST + 1e-3


@pytest.mark.parametrize("name", list(FIXTURES))
def test_ref_agrees_with_localba_ref(name):
    """LocalMapping's 5 + 10 iterations: the flags and their counts are localba_ref's; only the
    back-substitution order differs"""
    s = scene(**FIXTURES[name])
    a, b = ref(name, FULL), localba_ref.run_scene(s)
    m_chi, m_z = cr.margins(a, s["obs"])
    assert m_chi >= MARGIN and m_z >= MARGIN, name
    dev = deviation(a.Tcw, a.Xw, b)
    print(f"{name}: {dev:.4f} ulp from localba_ref, iterations {a.lm_iterations} / {[t.iterations for t in b.trace]}")
    assert a.rounds == b.rounds and np.array_equal(a.erase, b.erase) and np.array_equal(a.flag_first, b.flag_first)
    assert (a.n_bad_first, a.n_erase) == (b.n_bad_first, b.n_erase)


def test_scene_preconditions():
    """what the named fixtures are for holds"""
    assert [ref(n).n_free for n in ("f7", "f8", "f9")] == [[7, 7], [8, 8], [9, 9]] and NB == 48
    for n in ("f7", "f8", "f9"):
        s = scene(**FIXTURES[n])
        assert len(s["Tcw"]) == s["n_local"] + 2 and 55 <= len(s["Xw"]) <= 65
    s = scene(**FIXTURES["wide_pose"])
    assert np.bincount(s["pose_idx"])[:s["n_local"]].max() >= 257
    r = ref("all_flagged_pose")  # the second round's active set shrinks: a gap in hidx
    assert r.n_free == [3, 2] and not r.trace[1].iterations == 0
    st = localba_ref.structure(r.job, r.flag_first)
    assert list(st.hidx[:3]) == [0, -1, 1]
    r = ref("all_flagged_point")  # an inactive point
    assert r.n_active_points == [30, 29]
    r = ref("far_both")
    between = r.poll_kinds.index(cr.BETWEEN)
    assert cr.REJECTED in r.poll_kinds[:between] and cr.REJECTED in r.poll_kinds[between + 1:]
    assert r.lm_rejected[0] >= 1 and r.lm_rejected[1] >= 1 and limits("far_both") == FULL
    assert ref("e0").rounds == 0 and ref("e0").polls == 0
    assert cr.decisive(ref("far_both", THREAD_LIMITS)) and ref("far_both", THREAD_LIMITS).polls > r.polls


def test_ref_stop_at_every_poll():
    """stop_at = k for every k up to the polls of far_both: the three kinds of poll occur; poses and
    points equal a flagless run with the stopped run's iterations_applied as its limits; for a stop at
    the top of an iteration or between the rounds the erase flags are equal too (after a rejected trial
    the edges hold that trial's errors: the restatement's own counters only)"""
    full = ref("far_both")
    kinds = set()
    for k in range(full.polls + 1):
        a = ref("far_both", None, k)
        if k == full.polls:
            assert a.stop_poll == -1 and counters(a) == counters(full)
            continue
        kind = full.poll_kinds[k]
        kinds.add(kind)
        assert a.stop_poll == k and a.polls >= k + 1 and a.poll_kinds[:k + 1] == full.poll_kinds[:k + 1], k
        between = full.poll_kinds.index(cr.BETWEEN)
        rnd = 0 if k < between else 1
        if kind == cr.BETWEEN:
            assert a.rounds == 1 and a.stopped == [0, 0] and a.n_bad_first == 0 and not a.flag_first.any(), k
            assert a.lm_iterations[1] == 0 and a.iterations_applied[1] == 0
        else:
            assert a.stopped[rnd] == (1 if kind == cr.TOP else 2), k
            assert a.iterations_applied[rnd] == a.lm_iterations[rnd] - (1 if kind == cr.REJECTED else 0), k
            # a set flag stays set: the read between the rounds sees it after a stop in the first round
            assert a.rounds == (1 if rnd == 0 else 2), k
        second = a.iterations_applied[1] if a.rounds == 2 else 0
        b = ref("far_both", (a.iterations_applied[0], second))
        assert a.Tcw.tobytes() == b.Tcw.tobytes() and a.Xw.tobytes() == b.Xw.tobytes(), k
        if kind != cr.REJECTED and a.rounds == 2:
            assert np.array_equal(a.erase, b.erase) and np.array_equal(a.flag_first, b.flag_first), k
        if kind != cr.REJECTED and a.rounds == 1:
            # the flagless run classifies after its first round; with second = 0 its final flags are those
            assert np.array_equal(a.erase, b.erase), k
    assert kinds == {cr.TOP, cr.REJECTED, cr.BETWEEN}


def test_ref_stop_at_poll_0_leaves_the_depth_test_only():
    for name in ("far_both", "depth_only"):
        s, a = scene(**FIXTURES[name]), ref(name, None, 0)
        assert a.rounds == 1 and a.polls == 2 and a.lm_iterations == [0, 0] and a.stopped == [1, 0]
        assert (a.chi2_final == 0).all()
        z = localba_ref.edge_errors(*a.est, a.job)[2][2]
        assert np.array_equal(a.erase, ~(z > 0)), name
    assert ref("depth_only", None, 0).n_erase >= 1  # the point that starts behind its camera


def test_ref_no_second_round_leaves_the_first_flags():
    for name in ("p65", "all_flagged_pose", "far_both"):
        a = ref(name, (limits(name)[0], 0))
        assert a.rounds == 2 and a.lm_iterations[1] == 0 and np.array_equal(a.erase, a.flag_first) and a.n_bad_first == a.n_erase


# ---------------------------------------------------------------- CPU: argument checks of the library

ARRAYS = tuple(n for n, *_ in localba.INPUTS) + tuple(n for n, *_ in localba.OUTPUTS)


def _args(form, **kw):
    """the library call with fake non-null pointers (never dereferenced by a rejected call) and real edge
    indices for the host form's checks"""
    a = dict(P=3, NL=2, M=4, E=6, it1=5, it2=10, stop=None, stop_at=-1, res=1 << 20, ws=1 << 30, ws_bytes=1 << 40)
    a.update({name: 1 << (21 + k) for k, name in enumerate(ARRAYS)})
    a["edge_pose"] = np.array([0, 1, 2, 0, 1, 2], np.int32)
    a["edge_point"] = np.array([0, 0, 1, 2, 3, 3], np.int32)
    a.update(kw)
    ptr = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    arr = [ptr(a[n]) if form == "host" or a[n] is None else 1 << 23 for n in ARRAYS]
    L = localba._chip_lib()
    fn = L.orbgpu_local_ba_chip if form == "host" else L.orbgpu_local_ba_chip_device
    tail = () if form == "host" else (None,)
    return fn(a["P"], a["NL"], a["M"], a["E"], *arr[:8], a["it1"], a["it2"], a["stop"], a["stop_at"], *arr[8:], a["res"],
              a["ws"], a["ws_bytes"], *tail)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_checks_need_no_device(form):
    """rejected on the host before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    for name in ("P", "NL", "M", "E", "it1", "it2"):
        assert _args(form, **{name: -1}) == E, name
    assert _args(form, NL=4) == E and "n_local" in orbgpu.last_error()
    assert _args(form, stop_at=-2) == E and "stop_at_poll" in orbgpu.last_error()
    for name in (*ARRAYS, "res"):
        assert _args(form, **{name: None}) == E, name
        assert "null" in orbgpu.last_error(), name
    need = localba.chip_workspace_bytes(3, 2, 4, 6)
    assert need > 0 and need % 8 == 0
    assert _args(form, ws_bytes=need - 1) == E and "workspace" in orbgpu.last_error()
    assert _args(form, ws=(1 << 30) + 4) == E
    assert _args(form, P=2 ** 31 - 1, NL=2 ** 31 - 1) == E  # does not fit a size_t
    if form == "device":
        assert _args(form, ws=None) == E
    W = localba.chip_workspace_bytes
    assert W(-1, 0, 0, 0) == 0 and W(1, -1, 0, 0) == 0 and W(0, 0, -1, 0) == 0 and W(0, 0, 0, -1) == 0
    assert W(2, 3, 0, 0) == 0 and W(2 ** 31 - 1, 2 ** 31 - 1, 1, 1) == 0
    assert W(4, 2, 4, 6) > need > W(3, 2, 4, 5)
    # the dense reduced system is sized by the local poses alone: (6 NL + 1) 6 NL doubles
    assert W(300, 300, 0, 0) - W(300, 299, 0, 0) > 8 * 6 * 6 * 599 > W(301, 299, 0, 0) - W(300, 299, 0, 0)


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
    """(size, {member: offset}) of a struct of ints of include/orbgpu_localba_chip.h, from its text"""
    text = (ROOT / "include" / "orbgpu_localba_chip.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, offsets = 0, {}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        assert ctype == "int"
        for member in rest.split(","):
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", member.strip())
            offsets[m.group(1)] = off
            off += 4 * int(m.group(2) or 1)
    return off, offsets


def test_python_wrapper_and_struct_layout():
    """sizes and offsets agree between ctypes, the numpy dtype and the header"""
    R, D = localba.LocalBAChipResult, localba.CHIP_RESULT_DTYPE
    hsize, hoff = _header_struct("orbgpu_localba_chip_result")
    assert ctypes.sizeof(R) == D.itemsize == hsize == 72
    assert [f[0] for f in R._fields_] == list(D.names) == list(hoff)
    for field in D.names:
        assert getattr(R, field).offset == D.fields[field][1] == hoff[field], field
    s = scene(**FIXTURES["p2"])
    with pytest.raises(ValueError):
        localba.local_ba_chip(s["Tcw"], s["fixed"][:-1], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"], s["obs"],
                              s["inv_sigma2"], s["n_local"])


@pytest.fixture(scope="module")
def chip_args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("localba_chip_args") / "localba_chip_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "localba_chip_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(chip_args_main):
    """argument checks, the edge index checks of the host form and the workspace layout, compiled for the
    host with -fsanitize=address,undefined as a program of its own; its struct agrees with ctypes"""
    r = subprocess.run([str(chip_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
    r = subprocess.run([str(chip_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = {k: int(v) for k, v in re.findall(r"(\S+) (\d+)", r.stdout)}
    R = localba.LocalBAChipResult
    want = {name: getattr(R, name).offset for name, _ in R._fields_}
    want["orbgpu_localba_chip_result"] = ctypes.sizeof(R)
    assert got == want


# ---------------------------------------------------------------- GPU

def _torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


G = 64  # guard bytes around every device array


def _guarded(torch, a, fill=None):
    """a device copy of `a` (or `fill` bytes in its shape) between two runs of G guard bytes"""
    host = np.array(a, order="C")
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


def run_device(s, iterations, stream=None, stop=None, stop_at_poll=-1, workspace=None, mutate=None, before_call=None):
    """the device form on guarded copies, outputs and workspace pre-filled with 0x5A; returns (record,
    Tcw_out (n_local, 16), Xw_out (M, 3), erase (E), workspace triple); checks the guards and that no input
    changed"""
    torch = _torch_gpu()
    _, a = localba.make_batch([s])
    if mutate:
        mutate(a)
    tp, tm, te, nl = len(a["Tcw"]), len(a["Xw"]), len(a["obs"]), int(s["n_local"])
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d_in = [_guarded(torch, a[n]) for n, *_ in localba.INPUTS]
        d_T = _guarded(torch, np.zeros((nl, 16), F32), 0x5A)
        d_X = _guarded(torch, np.zeros((tm, 3), F32), 0x5A)
        d_E = _guarded(torch, np.zeros(te, np.uint8), 0x5A)
        ws = workspace or _guarded(torch, np.zeros(localba.chip_workspace_bytes(tp, nl, tm, te), np.uint8), 0x5A)
        before = [f.clone() for f, *_ in d_in]
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    if before_call:
        before_call()
    res = localba.local_ba_chip_device(*(v for _, v, _ in d_in), nl, d_T[1], d_X[1], d_E[1], ws[1], iterations,
                                       stream=stream, stop=stop, stop_at_poll=stop_at_poll)
    torch.cuda.synchronize()
    for (f, *_), b in zip(d_in, before):
        assert torch.equal(f, b)
    _guards_intact(d_in + [d_T, d_X, d_E, ws])
    return res, d_T[1].cpu().numpy(), d_X[1].cpu().numpy(), d_E[1].cpu().numpy(), ws


def record(res):
    return (tuple(tuple(int(v) for v in res[c]) for c in COUNTERS + SETS) + tuple(int(res[c]) for c in SCALARS))


def check_against_ref(res, T, X, erase, r, label, lm_counters=True):
    """the record, every local pose, point and erase byte against the restatement; the deviation in ulps"""
    bound = bound_of(label.split()[0])
    dev = deviation(T, X, r) if len(T) or len(X) else 0.0
    print(f"{label}: deviation {dev:.3f} ulp (bound {bound:.3f}), record {record(res)}; restatement {counters(r)}")
    assert res["status"] == 0 and T.shape == (len(r.Tcw), 16) and X.shape == r.Xw.shape and erase.shape == r.erase.shape
    assert set(np.unique(erase)) <= {0, 1}, label
    assert np.array_equal(erase.astype(bool), r.erase), (label, int((erase.astype(bool) != r.erase).sum()))
    if lm_counters:
        assert record(res) == counters(r), label
    else:  # decisions at rounding noise: the LM counters in range, everything else equal
        n = len(COUNTERS)
        assert record(res)[n:n + 2] == counters(r)[n:n + 2], label
        assert record(res)[n + 2:n + 5] == counters(r)[n + 2:n + 5], label
        for k in range(2):
            assert 0 <= res["lm_iterations"][k] <= FULL[k] and 0 <= res["lm_rejected"][k] <= 10 * FULL[k], label
    assert dev <= bound, (label, dev)
    assert np.array_equal(T[:, 12:], np.tile(F32([0, 0, 0, 1]), (len(T), 1))), label
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_gpu_fixture(name):
    """every fixture through the device form at its decisive limits: poses, points, erase flags and every
    counter; a fixture whose limits are shortened also at 5 + 10, the LM counters then in range only"""
    s, r = scene(**FIXTURES[name]), ref(name)
    check_margins(r, s, name)
    res, T, X, erase, _ = run_device(s, limits(name))
    check_against_ref(res, T, X, erase, r, name)
    if limits(name) != FULL:
        r = ref(name, FULL)
        m_chi, m_z = cr.margins(r, s["obs"])
        assert m_chi >= MARGIN and m_z >= MARGIN
        res, T, X, erase, _ = run_device(s, FULL)
        check_against_ref(res, T, X, erase, r, f"{name} at 5 + 10", lm_counters=False)


@pytest.mark.gpu
def test_gpu_host_form_determinism_and_a_used_workspace():
    """the host form gives the device form's bytes; two calls give equal bytes, the second on the workspace
    the first left"""
    for name in ("all_flagged_pose", "f9", "e0"):
        s = scene(**FIXTURES[name])
        res, T, X, erase, ws = run_device(s, limits(name))
        res2, T2, X2, erase2, _ = run_device(s, limits(name), workspace=ws)
        assert res.tobytes() == res2.tobytes() and T.tobytes() == T2.tobytes() and X.tobytes() == X2.tobytes()
        assert erase.tobytes() == erase2.tobytes()
        T1, X1, erase1, res1 = localba.local_ba_chip(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"],
                                                     s["obs"], s["inv_sigma2"], s["n_local"], limits(name))
        assert T1.tobytes() == T.tobytes() and X1.tobytes() == X.tobytes() and erase1.tobytes() == erase.tobytes()
        assert res1.tobytes() == res.tobytes(), name


@pytest.mark.gpu
def test_gpu_device_form_on_a_stream():
    torch = _torch_gpu()
    s = scene(**FIXTURES["f8"])
    res, T, X, erase, _ = run_device(s, limits("f8"), stream=torch.cuda.Stream())
    check_against_ref(res, T, X, erase, ref("f8"), "f8 on a stream")


@pytest.mark.gpu
def test_gpu_stop_at_poll_of_each_kind():
    """stop_at_poll = k for the first poll of each kind in the restatement's trace, and for poll 0"""
    s, full = scene(**FIXTURES["far_both"]), ref("far_both")
    between = full.poll_kinds.index(cr.BETWEEN)
    ks = {0, full.poll_kinds.index(cr.REJECTED), between, between + 1 + full.poll_kinds[between + 1:].index(cr.REJECTED),
          between + 1 + full.poll_kinds[between + 1:].index(cr.TOP) + 1}
    for k in sorted(ks):
        r = ref("far_both", None, k)
        check_margins(r, s, k)
        res, T, X, erase, _ = run_device(s, FULL, stop_at_poll=k)
        assert res["stop_poll"] == k
        check_against_ref(res, T, X, erase, r, f"far_both stop_at_poll={k} ({full.poll_kinds[k]})")


@pytest.mark.gpu
def test_gpu_stop_flag():
    """already set: poll 0 sees it.  Set from a second thread while far_both runs with larger limits:
    whatever stop_poll comes back, a call with stop_at_poll = stop_poll and no flag gives the same bytes,
    and the restatement with that stop_at agrees"""
    s = scene(**FIXTURES["far_both"])
    res, T, X, erase, _ = run_device(s, FULL, stop=globalba.StopFlag(True))
    assert res["stop_poll"] == 0
    check_against_ref(res, T, X, erase, ref("far_both", None, 0), "far_both flag set before the call")
    flag, go = globalba.StopFlag(), threading.Event()
    t = threading.Thread(target=lambda: (go.wait(), sum(range(20000)), flag.set()))
    t.start()  # it waits for the call to begin, which releases the interpreter lock to it
    res, T, X, erase, _ = run_device(s, THREAD_LIMITS, stop=flag, before_call=go.set)
    t.join()
    k = int(res["stop_poll"])
    print(f"flag from a second thread: stop_poll {k} of {res['polls']} polls")
    res2, T2, X2, erase2, _ = run_device(s, THREAD_LIMITS, stop_at_poll=k)
    assert res.tobytes() == res2.tobytes() and T.tobytes() == T2.tobytes() and X.tobytes() == X2.tobytes()
    assert erase.tobytes() == erase2.tobytes()
    r = ref("far_both", THREAD_LIMITS, k if k >= 0 else None)
    check_margins(r, s, k)
    check_against_ref(res, T, X, erase, r, f"far_both flag seen at poll {k}")


@pytest.mark.gpu
def test_gpu_nan_pose_ends_inside_the_pass_bound():
    s = scene(**FIXTURES["f7"])

    def mutate(a):
        a["Tcw"] = a["Tcw"].copy()
        a["Tcw"][1, 3] = np.nan

    res, T, X, erase, _ = run_device(s, FULL, mutate=mutate)
    print(f"NaN pose: record {record(res)}")
    assert res["status"] == 0 and res["rounds"] in (1, 2)
    for k in range(2):
        assert 0 <= res["lm_iterations"][k] <= FULL[k] and res["lm_rejected"][k] <= 10 * FULL[k]
    assert set(np.unique(erase)) <= {0, 1}


@pytest.mark.gpu
def test_gpu_bad_index_is_rejected_and_nothing_is_written():
    s = scene(**FIXTURES["e65"])
    for key, at, value in (("edge_pose", 40, len(s["Tcw"])), ("edge_pose", 0, -1), ("edge_point", 64, len(s["Xw"])),
                           ("edge_point", 30, 0)):
        def mutate(a, key=key, at=at, value=value):
            a[key] = a[key].copy()
            a[key][at] = value
        res, T, X, erase, _ = run_device(s, FULL, mutate=mutate)
        assert res["status"] == -1 and res["rounds"] == 0 and res["polls"] == 0, (key, at)
        assert (T.view(np.uint8) == 0x5A).all() and (X.view(np.uint8) == 0x5A).all() and (erase == 0x5A).all(), (key, at)


# ---------------------------------------------------------------- the C++ adapter and the map-mirror chain

from test_localba import _adapter_world, _check_marks, _run_adapter  # noqa: E402  (the stand-in world is shared)


@pytest.fixture(scope="module")
def localba_chip_main(tmp_path_factory):
    """tests/cpp/localba_chip_main.cpp against LocalBundleAdjuster.h and the cvlite stand-ins, one g++ line"""
    pkg = ROOT / "orb-slam2-annotation_amd"
    exe = tmp_path_factory.mktemp("localba_chip") / "localba_chip_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'tests' / 'cpp'}", '-DORBGPU_CV_HEADER="cvlite.hpp"', "-pthread", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "localba_chip_main.cpp"), f"-L{pkg}", "-lorbgpu", f"-Wl,-rpath,{pkg}"],
                   check=True)
    return exe


def test_adapter_builds_and_a_flag_set_before_the_call_touches_nothing(localba_chip_main, tmp_path):
    """LocalBundleAdjustmentChipGPU compiles against the stand-ins with -Wall -Wextra -Werror; with
    *pbStopFlag set it returns at :754-756 after the gather's marks: no device, no call on a keyframe, a
    MapPoint or the map; so does a neighbourhood without a local MapPoint"""
    s = scene(**SIZES["p15"])
    blob, problem, pose_kfs, point_order, marks = _adapter_world(s, np.random.default_rng(5))
    blob[3] = 1.0
    lines = _run_adapter(localba_chip_main, tmp_path, blob)
    assert {l[0] for l in lines} == {"B", "b"}
    _check_marks(lines, marks, int(blob[0]), int(blob[1]))
    blob, problem, pose_kfs, point_order, marks = _adapter_world(s, np.random.default_rng(5), with_points=False)
    assert {l[0] for l in _run_adapter(localba_chip_main, tmp_path, blob)} == {"B", "b"}


@pytest.mark.gpu
@pytest.mark.parametrize("name,flag", [("p65", 0.0), ("p17_kf0", -1.0)])
def test_gpu_adapter(localba_chip_main, tmp_path, name, flag):
    """LocalBundleAdjustmentChipGPU on test_localba.py's stand-in world (a clear flag, and a null
    pbStopFlag): the erased observations in the reference's order, every SetPose and SetWorldPos value,
    the call order and the marks, against the restatement run on what the gather must produce"""
    _torch_gpu()
    s = scene(**SIZES[name])
    blob, problem, pose_kfs, point_order, marks = _adapter_world(s, np.random.default_rng(3))
    blob[3] = flag
    r = cr.run_scene(problem)
    m_chi, m_z = cr.margins(r, problem["obs"])
    assert m_chi >= MARGIN and m_z >= MARGIN
    lines = _run_adapter(localba_chip_main, tmp_path, blob)
    calls = [l for l in lines if l[0] not in "Bb"]
    stereo = problem["obs"][:, 2] >= 0
    erased = [e for e in np.nonzero(r.erase & ~stereo)[0]] + [e for e in np.nonzero(r.erase & stereo)[0]]
    if name == "p65":
        assert len(erased) > 0
    expect = []
    for e in erased:
        k, m = pose_kfs[problem["pose_idx"][e]], point_order[problem["point_idx"][e]]
        expect += [["M", str(k), str(m)], ["O", str(m), str(k)]]
    n_er = len(expect)
    assert calls[:n_er] == expect
    NL, M = problem["n_local"], len(point_order)
    rest = calls[n_er:]
    assert [l[0] for l in rest] == ["P"] * NL + ["W", "U"] * M
    hexf = lambda words: np.array([int(w, 16) for w in words], np.uint32).view(F32)
    T = np.stack([hexf(l[2:]) for l in rest[:NL]])
    X = np.stack([hexf(l[2:]) for l in rest[NL::2]])
    assert [int(l[1]) for l in rest[:NL]] == pose_kfs[:NL]
    assert [int(l[1]) for l in rest[NL::2]] == point_order == [int(l[1]) for l in rest[NL + 1::2]]
    dev = deviation(T, X, r)
    print(f"adapter {name}: deviation {dev:.3f} ulp, {len(erased)} erased")
    assert dev <= bound_of(name)
    _check_marks(lines, marks, int(blob[0]), int(blob[1]))


@pytest.mark.gpu
def test_gpu_map_chain_with_the_chip_solve():
    """MapLocalBA.solve(chip=True) between gather() and collect() on the smallest converted scene, one
    job: after the collection vToErase and the scattered mirror rows are those of the restatement run
    on the gathered arrays; a job the gather rejected makes no call"""
    torch = _torch_gpu()
    import localba_map_ref as lr
    import localba_map_scene as ls
    import track
    for name in ("p1", "p65"):
        s = scene(**SIZES[name])
        sc = ls.from_problem(s)
        P, M, E, NL = len(s["Tcw"]), len(s["Xw"]), len(s["obs"]), s["n_local"]
        strides = dict(kf_stride=NL + 1, pose_stride=P + 2, point_stride=M + 3, edge_stride=E + 5)
        g = lr.gather(sc["mirror"], sc["ba"], 0, **strides)
        assert g.status == lr.OK and g.n_edges == E
        r = cr.local_bundle_adjustment(g.Tcw, g.fixed, g.cam, g.Xw, g.edge_pose, g.edge_point, g.obs, g.inv_sigma2,
                                       g.n_local)
        m_chi, m_z = cr.margins(r, np.asarray(g.obs, F32).reshape(-1, 3))
        assert m_chi >= MARGIN and m_z >= MARGIN
        mirror, ba = track.MapMirror(**sc["mirror"]), localba.MapMirrorBA(**sc["ba"])
        B = localba.MapLocalBA(mirror, ba, [0], **strides)
        B.chip_workspace()
        for key, t in B.t.items():
            if key not in ("gather_jobs", "chip_ws"):
                t.view(torch.uint8).fill_(0x5A)
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        B.gather(stream)
        B.solve(stream, chip=True, stop=globalba.StopFlag())
        B.collect(stream, write_mirror=True)
        stream.synchronize()
        res = B.chip_result
        assert res is not None and res["status"] == 0 and res["rounds"] == r.rounds and res["n_erase"] == r.n_erase
        erase = B.host("erase")[:E]
        assert np.array_equal(erase.astype(bool), r.erase)
        want = lr.collect(g, r.erase.astype(np.uint8))
        n = int(B.host("n_erase")[0])
        assert n == len(want) and [tuple(int(v) for v in row) for row in B.host("to_erase")[0][:n]] == want
        after_T = ba.t["kf_Tcw"].cpu().numpy().view(F32).reshape(-1, 12)
        after_X = mirror.t["pos"].cpu().numpy().view(F32).reshape(-1, 3)
        T = np.zeros((g.n_local, 4, 4), F32)
        T[:, 3, 3] = 1
        T[:, :3] = after_T[g.local_kfs].reshape(-1, 3, 4)
        dev = deviation(T, after_X[g.local_points], r)
        print(f"map chain {name}: deviation {dev:.3f} ulp, {n} erased, record {record(res)}")
        assert dev <= bound_of(name)
    # a job the gather rejected (pKF out of range): no call is made, nothing is solved
    B = localba.MapLocalBA(mirror, ba, [10 ** 6], **strides)
    B.chip_workspace()
    B.gather()
    B.solve(chip=True)
    assert B.chip_result is None
