"""Essential-graph optimisation (include/orbgpu_essential.h, csrc/essential.hip)
against the numpy restatement of Optimizer::OptimizeEssentialGraph
(tests/essential_ref.py) on the seeded loops of tests/essential_scene.py.

Parity: every element of Tcw_out and every point coordinate within ULP_BOUND
float32 ulps at the scale max(1, max|.|) of its array; Scw_out's doubles are
compared in the same way, the bound expressed in float32 ulps.  The kernels and
the restatement write the same expressions and add every sum in the same order,
so what is left is exp / log / sin / cos / acos (libm here, the device library
there).  The Jacobians are 1e-9 central differences, which magnify a rounding
of the error by 5e8, so the bound is measured, not fixed (the rule of
test_sim3opt.py): MEASURED_WORST is the largest deviation the restatement shows
on any fixture under 8 permutations of the edge order, 8 permutations of the
keyframe order and 8 seeded runs in which every result of the five functions is
moved by up to 2 ulp (by a seeded hash of the argument), and ULP_BOUND = max(2, 4 x MEASURED_WORST).
test_ref_permutation_spread_of_every_fixture asserts the measurement.

iterations, rejected, n_free and n_active_edges are compared for equality: every
fixture's seed and iteration count are chosen on the CPU so that every decision
of the restatement (accept or reject, rho == 0, the stop criterion, every branch
of Sim3(Vector7d) and Sim3::log) stays 1e-6 (relative) from its threshold, under
each of the 24 variations too; the tests assert that (essential_ref.decisive)
before they compare.

Measured on the CPU, the restatement under the 24 variations: 0.0-0.96 ulp on
the fixtures whose second iteration is rejected, 0.4-15.0 on those with two
accepted iterations, 34.7 on the far start, so the bound is 138.8 ulp.  Measured
on an MI355X against the restatement: 9.7 ulp on the far start, 3.6 on f16, 2.6
on f6, 2.5 on dup, 1.9 on f7, 1.8 on e65, below 1 on the other 16 fixtures, 4.6
and 1.5 through the C++ adapter, with the four integers equal everywhere
(DESIGN.md §5o).
"""
import ctypes
import functools
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import essential
import essential_ref as er
import essential_scene as es
import globalba_ref
import orbgpu

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
ULP = 2.0 ** -23
VARIATIONS = 8
NB = 48  # csrc/chol_blocked.h: kNB, the panel width of the blocked Cholesky
# the restatement's worst deviation under the 24 variations of any fixture, in float32 ulp, measured on the
# CPU (the largest: `far`)
MEASURED_WORST = 34.7
ULP_BOUND = max(2.0, 4.0 * MEASURED_WORST)

# name: (scene, n_iterations).  Free active vertices F in {1, 6, 7, 14, 16} with keyframe 0 fixed (7, 42, 49,
# 98 and 112 unknowns: either side of one and two 48-wide panels, and 65 rows below the first panel, one
# past kRows); e*: the edge counts around the wave and the workgroup; fix_*: the fixed vertex first, in the
# middle, last, and two fixed vertices with an edge between them; gap: keyframe 4 without an edge between
# keyframes that have some; dup: three and two edges between one pair in both orientations and kinds;
# star: keyframe 3 with 260 incident edges; tables: keyframes with a corrected Sim3, a non-corrected one,
# both or neither; far: a far start (0.3 rad, 0.9 m) whose run has accepted and rejected trials
FIXTURES = {
    "f1": (dict(n_kf=2, seed=101, fix_scale=1, n_corrected=1), 1),
    "f6": (dict(n_kf=7, seed=102, fix_scale=0), 2),
    "f7": (dict(n_kf=8, seed=203, fix_scale=1), 2),
    "f14": (dict(n_kf=15, seed=904, fix_scale=0), 2),
    "f16": (dict(n_kf=17, seed=305, fix_scale=1), 2),
    "e0": (dict(n_kf=10, seed=110, fix_scale=1, n_edges=0), 3),
    "e1": (dict(n_kf=10, seed=111, fix_scale=0, n_edges=1, lead=((9, 0, 1),)), 1),
    "e63": (dict(n_kf=10, seed=212, fix_scale=1, n_edges=63), 2),
    "e64": (dict(n_kf=10, seed=513, fix_scale=0, n_edges=64), 2),
    "e65": (dict(n_kf=10, seed=214, fix_scale=1, n_edges=65), 2),
    "e255": (dict(n_kf=10, seed=115, fix_scale=0, n_edges=255), 2),
    "e256": (dict(n_kf=10, seed=516, fix_scale=1, n_edges=256), 2),
    "e257": (dict(n_kf=10, seed=3517, fix_scale=0, n_edges=257), 2),
    "fix_mid": (dict(n_kf=10, seed=120, fix_scale=1, fixed=(5,)), 2),
    "fix_last": (dict(n_kf=10, seed=321, fix_scale=0, fixed=(9,)), 2),
    "fix_pair": (dict(n_kf=10, seed=222, fix_scale=1, fixed=(0, 1)), 2),
    "gap": (dict(n_kf=10, seed=123, fix_scale=0, strip=4, lead=((5, 3, 1),)), 2),
    "dup": (dict(n_kf=10, seed=324, fix_scale=1, multi=((2, 5, 3), (8, 6, 3), (3, 6, 2))), 2),
    "star": (dict(n_kf=17, seed=125, fix_scale=0, star=(3, 260)), 2),
    "tables": (dict(n_kf=10, seed=226, fix_scale=0, c_only=(2,), nc_only=(4,)), 2),
    "far": (dict(n_kf=10, seed=327, fix_scale=0, start=0.3), 4),
}
SEAMS = ("f1", "f6", "f7", "f14", "f16")
COUNTERS = ("iterations", "rejected", "n_free", "n_active_edges")


def scene(name, **more):
    return es.scene(**{**FIXTURES[name][0], **more})


@functools.lru_cache(maxsize=None)
def ref(name, n_iterations=None):
    """the restatement's result of a fixture, computed once per session"""
    it = FIXTURES[name][1]
    return er.run_scene(scene(name), it if n_iterations is None else n_iterations)


def varied(name, kind, k):
    """the restatement on a fixture with its edges permuted, its keyframes permuted, or the five functions
    nudged by up to 2 ulp"""
    s, it = scene(name), FIXTURES[name][1]
    if kind == "edges":
        return er.run_scene(s, it, edge_perm=np.random.default_rng(1000 + k).permutation(len(s["edge_i"])))
    if kind == "keyframes":
        return er.run_scene(s, it, kf_perm=np.random.default_rng(2000 + k).permutation(len(s["Tcw"])))
    return er.run_scene(s, it, fn=er.NudgedFn(3000 + k, 2))


def _ulps(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if len(b) == 0:
        return 0.0
    scale = max(1.0, float(np.abs(b[np.isfinite(b)]).max()) if np.isfinite(b).any() else 1.0)
    with np.errstate(all="ignore"):
        diff = np.abs(a - b)
    diff = np.where(np.isnan(a) & np.isnan(b), 0.0, diff)
    return float(diff.max()) / (ULP * scale)


def deviation(S, T, X, r):
    """largest deviation of Scw (N, 8), Tcw (N, 4, 4) float32 and Xw (M, 3) float32 from the restatement's,
    in float32 ulps at the scale max(1, max|.|) of each array"""
    return max(_ulps(np.asarray(S).reshape(-1, 8), r.Scw), _ulps(np.asarray(T).reshape(-1, 4, 4), r.Tcw),
               _ulps(X, r.Xw))


def round_trip(s):
    """what a call writes when nothing is optimised"""
    return er.run_scene(s, 0)


# ---------------------------------------------------------------- CPU: the restatement's own checks

THETA_LOG = float(np.arccos(er.ONE_MINUS_EPS))  # Sim3::log's d > 1 - eps in terms of the angle: 4.47e-3


@pytest.mark.parametrize("sigma", [0.0, 0.5e-5, -0.5e-5, 2e-5, 0.3, -0.2])
@pytest.mark.parametrize("theta", [0.0, 0.5e-5, 2e-5, 0.5 * THETA_LOG, 2 * THETA_LOG, 0.7])
def test_ref_log_inverts_exp_around_every_branch(sigma, theta):
    """log(Sim3(u)) = u on both sides of |sigma| < 1e-5, of theta < 1e-5 (Sim3(Vector7d)) and of d > 1 - 1e-5
    (Sim3::log), within the truncation of the series the branches taken use:
      omega     log's small-angle branch takes 0.5 deltaR(R) = (sin theta / theta) omega: theta^3 / 6
      upsilon   W differs between the two functions where one used A = 1/2, B = 1/6 (or their sigma forms)
                and the other the closed forms: |dA| theta + |dB| theta^2 on |upsilon|, dA <= theta^2 / 24,
                dB <= theta^2 / 120 for |sigma| < eps; for |sigma| >= eps the small-angle B as written lacks the
                series' -1: it is 1 / sigma^3 too large, which stands against the closed form wherever log
                takes its small-angle branch and Sim3(Vector7d) does not: theta^2 / |sigma|^3 on |upsilon|.
                Where both take the same branch the same W is built and solved: rounding times W's condition,
                and eps / |sigma| from the cancellation in C = (s - 1) / sigma
    """
    rng = np.random.default_rng(int(1e7 * abs(sigma) + 1e3 * theta) + 7)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    up = rng.standard_normal(3)
    u = [np.array([v]) for v in (*(theta * axis), *up, sigma)]
    fn = er.Fn()
    v = er.sim3_log(er.sim3_exp(u, fn), fn)
    err_om = max(abs(float(v[k][0] - u[k][0])) for k in range(3))
    err_up = max(abs(float(v[k][0] - u[k][0])) for k in range(3, 6))
    exp_small, log_small, big_sigma = theta < er.EPS, theta < THETA_LOG, abs(sigma) >= er.EPS
    written = 1.0 / abs(sigma) ** 3 if big_sigma else 0.0  # the as-written B against the closed form
    # W's size over its smallest pivot C ~ 1 where the as-written B rules it
    cond = 1.0 + (written * theta ** 2 if log_small else 0.0)
    tol_om = 64 * np.finfo(float).eps * max(1.0, cond) + (theta ** 3 / 6 if log_small else 0.0)
    n_up = float(np.linalg.norm(up))
    # C = (s - 1) / sigma cancels in s - 1, and log reads sigma back from s: eps / |sigma| of C each
    cancel = 8 * np.finfo(float).eps / abs(sigma) if big_sigma else 0.0
    if not exp_small:  # Sim3(Vector7d)'s closed forms cancel in 1 - cos(theta): eps / theta^2 of A, on theta |upsilon|
        cancel += 8 * np.finfo(float).eps / theta
    tol_up = (1e3 * np.finfo(float).eps * cond * cond + cancel * cond) * n_up + 2 * tol_om * n_up
    if log_small and not exp_small:
        tol_up += (theta ** 3 / 24 + theta ** 4 / 120 + (written + (1.0 if big_sigma else 0.0)) * theta ** 2) * n_up * 1.5
    print(f"sigma {sigma:g} theta {theta:g}: omega off by {err_om:.3g} (bound {tol_om:.3g}), upsilon by {err_up:.3g} "
          f"(bound {tol_up:.3g})")
    assert abs(float(v[6][0]) - sigma) <= 4 * np.finfo(float).eps * max(1.0, abs(sigma))
    assert err_om <= tol_om and err_up <= tol_up
    if big_sigma and log_small and not exp_small and 1e-9 < written * theta ** 2 < 0.1:
        # the as-written B is kept: the closed form's round trip would be exact to rounding
        assert err_up > 0.05 * written * theta ** 2 * n_up / 3


def test_ref_numeric_jacobian_against_the_complex_step():
    """BaseBinaryEdge::linearizeOplus' central differences against the complex-step derivative of the same
    error (the restatement's own expressions on complex numbers, step 1e-30: no cancellation).  The
    central difference's own noise: an error evaluation is some tens of operations on values up to the
    translations' size m, each rounded to eps m; two of them over 2e-9: 64 eps m / 2e-9.  Its truncation,
    delta^2 / 6 times a third derivative, is below 1e-17."""
    s = scene("f7", fix_scale=0)
    job = er.make_job(*(s[k] for k in er.ARRAYS), 0)
    fn = er.Fn()
    est = [c.copy() for c in job.vScw]
    A, B = er.jacobians(est, job, fn)
    ae, vi, vj = job.ae, job.ei[job.ae], job.ej[job.ae]
    C = er.take(job.meas, ae)
    inv = er.sim3_inverse(est)
    m = max(1.0, float(np.abs(np.stack(est[4:7])).max()))
    bound = 64 * np.finfo(float).eps * m / (2 * er.DELTA)
    worst = 0.0
    h = 1e-30
    for d in range(7):
        u = [np.zeros(job.n, complex) for _ in range(7)]
        u[d] = u[d] + 1j * h
        with np.errstate(all="ignore"):
            P = er.oplus([c.astype(complex) for c in est], u, 0, fn)
            Pinv = er.sim3_inverse(P)
            ea = er.edge_error(C, er.take(P, vi), er.take(inv, vj), fn)
            eb = er.edge_error(C, er.take(est, vi), er.take(Pinv, vj), fn)
        for r in range(7):
            fi, fj = ~job.fixed[vi], ~job.fixed[vj]
            worst = max(worst, float(np.abs(A[:, r, d] - ea[r].imag / h)[fi].max()),
                        float(np.abs(B[:, r, d] - eb[r].imag / h)[fj].max()))
    print(f"numeric Jacobian off the complex step by {worst:.3g} (noise bound {bound:.3g})")
    assert 0 < worst <= bound


def test_ref_drift_free_graph_does_not_move():
    """corrected Sim3s equal to the non-corrected ones: every measurement is met.  The poses are float32
    matrices, orthonormal to 2^-24, and Quaterniond(Matrix3d), the products and conjugate() as inverse
    never normalise: an error is 2^-24 times a few on the rotation and that times the translations' size m
    on the translation, so chi2 is below (8 2^-24 m)^2 per edge and no estimate moves by more than that"""
    s = es.scene(10, 7, fix_scale=0, consistent=True)
    r = er.run_scene(s, 5)
    m = max(1.0, float(np.abs(r.job.vScw[4:7]).max()))
    level = 8 * 2.0 ** -24 * m
    assert r.n_active_edges == len(s["edge_i"]) and 0 < r.first_chi <= r.n_active_edges * level ** 2
    assert r.last_chi <= r.first_chi
    moved = float(np.abs(r.Scw - er.as_rows(r.job.vScw)).max())
    print(f"drift-free: chi2 {r.first_chi:.3g} -> {r.last_chi:.3g}, moved {moved:.3g} (level {level:.3g})")
    assert moved <= 4 * level


def test_ref_loop_spreads_the_correction_over_the_edges():
    """exact measurements between the non-corrected poses, only the corrected set disagrees: at the start
    the whole chi2 sits on the normal edges between a corrected and an uncorrected keyframe; at the end the sum
    is lower and every edge's chi2 is below the largest any edge started with"""
    s = es.scene(12, 8, fix_scale=0)
    r = er.run_scene(s, 10)
    first, last = r.trace.edge_chi_first, r.trace.edge_chi_last
    corrected = s["has_corrected"].astype(bool)
    # a LoopConnections edge is measured between the corrected poses themselves: it starts at zero too
    inner = (corrected[s["edge_i"]] == corrected[s["edge_j"]]) | (s["edge_kind"] == 0)
    assert (~inner).any() and first[inner].max() < 1e-9 < 1e-4 < first[~inner].min() and r.last_chi < 0.1 * r.first_chi
    assert last.max() < first.max() and (last[~inner] < first[~inner]).all()


@pytest.mark.parametrize("name", ["far", "f14", "f16"])
def test_ref_every_accepted_trial_lowers_chi2(name):
    tr = ref(name).trace
    chi = tr.first_chi
    assert any(tr.trials) and len(tr.trials) == len(tr.chi_after)
    for accepted, after in zip(tr.trials, tr.chi_after):
        assert (after < chi) if accepted else (after == chi)
        chi = after


@pytest.mark.parametrize("name", [n for n, (kw, _) in FIXTURES.items() if kw["fix_scale"] and n != "e0"])
def test_ref_fix_scale_keeps_every_scale(name):
    """under fix_scale every seventh Jacobian column is exactly zero and every scale keeps its bits"""
    r = ref(name)
    assert r.iterations >= 1
    for sys in r.trace.systems:
        assert not sys.A[:, :, 6].any() and not sys.B[:, :, 6].any() and sys.A[:, :, :6].any()
        assert not sys.b.reshape(-1, 7)[:, 6].any()
    assert r.Scw[:, 7].tobytes() == np.asarray(r.job.vScw[7]).tobytes()
    assert (r.Scw[:, :7] != er.as_rows(r.job.vScw)[:, :7]).any()


def test_ref_edge_between_fixed_vertices_adds_nothing():
    s, r = scene("fix_pair"), ref("fix_pair")
    both = s["fixed"][s["edge_i"]].astype(bool) & s["fixed"][s["edge_j"]].astype(bool)
    assert both.sum() == 1 and r.n_active_edges == len(both) - 1
    t = dict(s)
    for k in ("edge_i", "edge_j", "edge_kind"):
        t[k] = s[k][~both]
    q = er.run_scene(t, FIXTURES["fix_pair"][1])
    assert q.n_active_edges == r.n_active_edges and q.first_chi == r.first_chi
    assert q.Scw.tobytes() == r.Scw.tobytes() and q.Tcw.tobytes() == r.Tcw.tobytes() and q.Xw.tobytes() == r.Xw.tobytes()


def test_ref_inactive_vertex_and_unreferenced_point_keep_their_bits():
    s, r = scene("gap"), ref("gap")
    rt = round_trip(s)
    assert not ((s["edge_i"] == 4) | (s["edge_j"] == 4)).any() and not s["fixed"][4] and r.n_free == 8
    for v in (0, 4):  # fixed, inactive: the unchanged estimate through the write-out
        assert r.Scw[v].tobytes() == er.as_rows(r.job.vScw)[v].tobytes() and r.Tcw[v].tobytes() == rt.Tcw[v].tobytes()
    assert all(r.Scw[v].tobytes() != rt.Scw[v].tobytes() for v in range(10) if v not in (0, 4))
    keep = s["point_ref"] < 0
    still = keep | np.isin(s["point_ref"], (0, 4))
    assert keep.any() and (~still).any()
    assert r.Xw[keep].tobytes() == s["Xw"][keep].tobytes()
    assert r.Xw[still].tobytes() == rt.Xw[still].tobytes() and (r.Xw[~still] != rt.Xw[~still]).any()


@pytest.mark.parametrize("n", [7, 42, 49, 98, 112])
def test_ref_blocked_order_solve_equals_the_unblocked_loop(n):
    """globalba_ref.blocked_order_solve at the sizes of the seam fixtures: L and y bit-equal to the
    unblocked loops of lm_ref.cholesky_solve, x to the column-oriented back-substitution written out"""
    rng = np.random.default_rng(n)
    Araw = rng.standard_normal((n, n))
    S = Araw @ Araw.T + np.eye(n)
    b = rng.standard_normal(n)
    x, L, y = globalba_ref.blocked_order_solve(S, b)
    Lr = np.zeros((n, n))
    for j in range(n):
        t = float(S[j][j])
        for k in range(j):
            t -= Lr[j][k] * Lr[j][k]
        Lr[j][j] = np.sqrt(t)
        for i in range(j + 1, n):
            t = float(S[i][j])
            for k in range(j):
                t -= Lr[i][k] * Lr[j][k]
            Lr[i][j] = t / Lr[j][j]
    yr = np.zeros(n)
    for i in range(n):
        t = float(b[i])
        for k in range(i):
            t -= Lr[i][k] * yr[k]
        yr[i] = t / Lr[i][i]
    sr, xr = yr.copy(), np.zeros(n)
    for i in range(n - 1, -1, -1):
        xr[i] = sr[i] / Lr[i][i]
        for k in range(i):
            sr[k] -= Lr[i][k] * xr[i]
    assert L.tobytes() == Lr.tobytes() and y.tobytes() == yr.tobytes() and x.tobytes() == xr.tobytes()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_ref_permutation_spread_of_every_fixture(name):
    """the same scene with its edges permuted, its keyframes permuted (every sum rounds differently) and
    with the five library functions nudged by up to 2 ulp, 8 times each: every run is decisive, the
    integer outcomes are equal, and the outputs stay within the measured worst the GPU bound is made from"""
    a = ref(name)
    assert er.decisive(a), (name, min(a.trace.margins + a.fn.margins))
    worst = {}
    for kind in ("edges", "keyframes", "nudged"):
        for k in range(VARIATIONS):
            b = varied(name, kind, k)
            assert er.decisive(b), (name, kind, k, min(b.trace.margins + b.fn.margins))
            assert all(getattr(a, c) == getattr(b, c) for c in COUNTERS), (name, kind, k)
            worst[kind] = max(worst.get(kind, 0.0), deviation(b.Scw, b.Tcw, b.Xw, a))
    print(f"{name}: spread " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          f" ulp; iterations {a.iterations}, rejected {a.rejected}")
    assert max(worst.values()) <= MEASURED_WORST <= ULP_BOUND / 4


def test_scene_preconditions():
    """what the named fixtures are for holds"""
    assert [ref(n).n_free for n in SEAMS] == [1, 6, 7, 14, 16]
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        assert len(scene(f"e{n}")["edge_i"]) == n
    assert ref("e0").iterations == 0 and ref("e1").n_free == 1 and ref("e1").iterations >= 1
    assert {FIXTURES[n][0]["fix_scale"] for n in FIXTURES} == {0, 1}
    assert {FIXTURES[n][0]["fix_scale"] for n in SEAMS} == {0, 1}
    for name, at in (("f7", 0), ("fix_mid", 5), ("fix_last", 9)):
        assert np.nonzero(scene(name)["fixed"])[0].tolist() == [at]
    assert ref("fix_pair").n_active_edges == len(scene("fix_pair")["edge_i"]) - 1
    s = scene("dup")
    pairs = {}
    for i, j, k in zip(s["edge_i"], s["edge_j"], s["edge_kind"]):
        pairs.setdefault((min(i, j), max(i, j)), []).append((int(i < j), int(k)))
    multi = sorted(len(v) for v in pairs.values() if len(v) > 1)
    assert multi[-1] >= 3 and len(multi) >= 2
    assert any(len(set(v)) >= 3 for v in pairs.values())  # orientations and kinds mixed within a pair
    s = scene("star")
    assert ((s["edge_i"] == 3) | (s["edge_j"] == 3)).sum() == 260
    s = scene("tables")
    assert {(int(c), int(n)) for c, n in zip(s["has_corrected"], s["has_noncorrected"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for name in FIXTURES:
        s = scene(name)
        refs = s["point_ref"]
        c = s["has_corrected"].astype(bool)
        assert (refs < 0).any() and c[refs[refs >= 0]].any() and (~c[refs[refs >= 0]]).any(), name
    tr = ref("far").trace
    assert tr.rejected >= 1 and sum(tr.trials) >= 3 and tr.first_chi > 100 * tr.last_chi


# ---------------------------------------------------------------- CPU: argument checks of the library

ARRAYS = tuple(n for n, *_ in essential.INPUTS) + tuple(n for n, *_ in essential.OUTPUTS)


def _args(form, **kw):
    """the library call with fake non-null pointers (never dereferenced by a rejected call) and real edge
    indices and point references for the host form's checks"""
    a = dict(N=4, E=5, M=3, fix=1, it=5, res=1 << 20, ws=1 << 30, ws_bytes=1 << 40)
    a.update({name: 1 << (21 + k) for k, name in enumerate(ARRAYS)})
    a["edge_i"] = np.array([1, 2, 3, 3, 0], np.int32)
    a["edge_j"] = np.array([0, 1, 2, 0, 2], np.int32)
    a["point_ref"] = np.array([0, -1, 3], np.int32)
    a.update(kw)
    ptr = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    arr = [ptr(a[n]) if form == "host" or a[n] is None else 1 << 23 for n in ARRAYS]
    L = essential._lib()
    fn = L.orbgpu_optimize_essential_graph if form == "host" else L.orbgpu_optimize_essential_graph_device
    tail = () if form == "host" else (None,)
    return fn(a["N"], a["E"], a["M"], *arr[:11], a["fix"], a["it"], *arr[11:], a["res"], a["ws"], a["ws_bytes"], *tail)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_checks_need_no_device(form):
    """rejected on the host before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    for name in ("N", "E", "M", "it"):
        assert _args(form, **{name: -1}) == E, name
    for name in (*ARRAYS, "res"):
        assert _args(form, **{name: None}) == E, name
        assert "null" in orbgpu.last_error(), name
    need = essential.workspace_bytes(4, 5, 3)
    assert need > 0 and need % 8 == 0
    assert _args(form, ws_bytes=need - 1) == E and "workspace" in orbgpu.last_error()
    assert _args(form, ws=(1 << 30) + 4) == E
    if form == "device":
        assert _args(form, ws=None) == E
    assert essential.workspace_bytes(-1, 0, 0) == 0 and essential.workspace_bytes(0, -1, 0) == 0
    assert essential.workspace_bytes(0, 0, -1) == 0
    assert essential.workspace_bytes(2 ** 31 - 1, 1, 1) == 0  # (7 N)^2 doubles do not fit a size_t
    assert essential.workspace_bytes(5, 5, 3) > need > essential.workspace_bytes(4, 4, 3)
    # the dense system: (7 N + 1) 7 N doubles
    assert essential.workspace_bytes(300, 0, 0) - essential.workspace_bytes(299, 0, 0) > 8 * 7 * 7 * 599


def test_index_checks_of_the_host_form_need_no_device():
    E = orbgpu.ERR_ARG
    for key, k, v, word in (("edge_i", 2, 4, "out of range"), ("edge_i", 0, -1, "out of range"),
                            ("edge_j", 4, 7, "out of range"), ("edge_j", 1, -2, "out of range"),
                            ("edge_j", 3, 3, "one keyframe"), ("point_ref", 2, 4, "point_ref")):
        arr = {"edge_i": [1, 2, 3, 3, 0], "edge_j": [0, 1, 2, 0, 2], "point_ref": [0, -1, 3]}[key]
        arr = np.array(arr, np.int32)
        arr[k] = v
        assert _args("host", **{key: arr}) == E and word in orbgpu.last_error(), (key, k, v)


def _header_struct(name):
    """(size, {member: offset}) of a struct of include/orbgpu_essential.h, from its text"""
    text = (ROOT / "include" / "orbgpu_essential.h").read_text()
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
            count = re.search(r"\[(\d+)\]", member)
            off = (off + size - 1) // size * size
            offsets[re.sub(r"\[.*", "", member).strip()] = off
            off += size * (int(count.group(1)) if count else 1)
    return off, offsets


def test_python_wrapper_and_struct_layout():
    """sizes and offsets agree between ctypes, the numpy dtype and the header"""
    hsize, hoff = _header_struct("orbgpu_eg_result")
    assert ctypes.sizeof(essential.EGResult) == essential.RESULT_DTYPE.itemsize == hsize == 56
    assert [f[0] for f in essential.EGResult._fields_] == list(essential.RESULT_DTYPE.names) == list(hoff)
    for field in essential.RESULT_DTYPE.names:
        assert getattr(essential.EGResult, field).offset == essential.RESULT_DTYPE.fields[field][1] == hoff[field], field
    s = scene("f7")
    with pytest.raises(ValueError):
        essential.pack(*(s[k] if k != "fixed" else s[k][:-1] for k in er.ARRAYS))


@pytest.fixture(scope="module")
def essential_args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("essential_args") / "essential_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "essential_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(essential_args_main):
    """argument checks, the index checks of the host form and the workspace layout, compiled for the host
    with -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(essential_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
    r = subprocess.run([str(essential_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = {k: int(v) for k, v in re.findall(r"(\S+) (\d+)", r.stdout)}
    R = essential.EGResult
    assert got == {"orbgpu_eg_result": ctypes.sizeof(R), "result.n_active_edges": R.n_active_edges.offset,
                   "result.first_chi2": R.first_chi2.offset, "result.last_lambda": R.last_lambda.offset}


# ---------------------------------------------------------------- the C++ adapter

@pytest.fixture(scope="module")
def essential_main(tmp_path_factory):
    """tests/cpp/essential_main.cpp against EssentialGraphOptimizer.h and the cvlite stand-ins, one g++ line"""
    pkg = ROOT / "orb-slam2-annotation_amd"
    exe = tmp_path_factory.mktemp("essential") / "essential_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'tests' / 'cpp'}", '-DORBGPU_CV_HEADER="cvlite.hpp"', "-pthread", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "essential_main.cpp"), f"-L{pkg}", "-lorbgpu", "-ldl",
                    f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def _adapter_world(s, rng, n_iterations, all_bad=False):
    """Stand-in keyframes and MapPoints around a scene's vertices (its edges are not used: the world has
    its own), with what the enumeration must skip or drop interleaved: a bad keyframe in the map and a
    keyframe that is not in the map (both are parents, loop-edge partners, covisible keyframes and
    reference keyframes of others), covisibility below 100, covisible parents, children, loop-edge
    partners and LoopConnections pairs, a LoopConnections pair below 100 and the pCurKF / pLoopKF pair that
    is kept whatever its weight, a bad MapPoint.  Keyframe indices are shuffled, so neither GetAllKeyFrames()
    nor the maps and sets (ordered by keyframe index) are in the scene's order.  Returns (blob for
    essential_main, the problem as the adapter must hand it to the library as a dict with the edge list,
    the keyframe index of each vertex, the MapPoints that are written)."""
    n = len(s["Tcw"])
    assert n >= 8 and np.nonzero(s["fixed"])[0].tolist() == [0]
    n_all = n + 2
    kf_of_vertex = [int(k) for k in rng.permutation(n_all)[:n]]
    bad_kf, out_kf = sorted(set(range(n_all)) - set(kf_of_vertex))
    loop, cur = kf_of_vertex[0], kf_of_vertex[n - 1]
    ids = {kf_of_vertex[v]: 3 * v + 2 for v in range(n)}
    ids[bad_kf], ids[out_kf] = 3 * 3 + 3, 3 * n + 7
    bad = {k: all_bad and k != out_kf for k in range(n_all)}
    bad[bad_kf] = True
    in_map = {k: k != out_kf for k in range(n_all)}
    K = lambda v: kf_of_vertex[v]
    parent = {k: -1 for k in range(n_all)}
    children = {k: set() for k in range(n_all)}
    loops = {k: set() for k in range(n_all)}
    cov = {k: {} for k in range(n_all)}

    def covisible(a, b, w):
        cov[a][b] = w
        cov[b][a] = w
    for v in range(1, n):
        parent[K(v)] = K(v - 1)
        children[K(v - 1)].add(K(v))
        covisible(K(v), K(v - 1), 200)                     # the parent / a child
        for back in (2, 3):
            if v - back >= 0 and rng.uniform() < 0.6:
                covisible(K(v), K(v - back), int(rng.integers(100, 300)))
        if v - 4 >= 0:
            covisible(K(v), K(v - 4), 50)                  # below minFeat
    parent[K(0)], parent[bad_kf] = out_kf, K(2)             # dropped: an end is no vertex
    for a, b in ((K(n // 2 + 1), K(1)), (bad_kf, K(3))):
        loops[a].add(b), loops[b].add(a)
    covisible(K(n // 2 + 1), K(1), 160)                     # a loop-edge partner
    covisible(K(4), bad_kf, 150), covisible(K(5), out_kf, 180)
    covisible(K(n - 1), K(1), 50), covisible(K(n - 1), K(2), 120), covisible(K(n - 2), K(0), 130)
    cov[cur].pop(loop, None), cov[loop].pop(cur, None)      # GetWeight(pCurKF, pLoopKF) = 0: kept all the same
    LC = {cur: {loop, K(1), K(2)}, K(n - 2): {K(0)}}
    by_weight = {k: [o for o, _ in sorted(cov[k].items(), key=lambda kv: -kv[1])] for k in range(n_all)}
    # the enumeration of src/Optimizer.cpp:989-1133 on this world
    good = [k for k in range(n_all) if in_map[k] and not bad[k]]
    vertex_of = {k: i for i, k in enumerate(good)}
    edges, inserted = [], set()

    def add(a, b, kind):
        if a in vertex_of and b in vertex_of:
            edges.append((vertex_of[a], vertex_of[b], kind))
    for key in sorted(LC):
        for other in sorted(LC[key]):
            if (ids[key] != ids[cur] or ids[other] != ids[loop]) and cov[key].get(other, 0) < 100:
                continue
            add(key, other, 0)
            inserted.add((min(ids[key], ids[other]), max(ids[key], ids[other])))
    for k in range(n_all):
        if not in_map[k]:
            continue
        if parent[k] >= 0:
            add(k, parent[k], 1)
        for l in sorted(loops[k]):
            if ids[l] < ids[k]:
                add(k, l, 1)
        for o in by_weight[k]:
            if cov[k][o] < 100 or o == parent[k] or o in children[k] or o in loops[k]:
                continue
            if bad[o] or not ids[o] < ids[k] or (min(ids[k], ids[o]), max(ids[k], ids[o])) in inserted:
                continue
            add(k, o, 1)
    # MapPoints: the scene's, each through one of the two ways to its reference, and a bad one
    pts = []  # (bad, X, mnCorrectedByKF, mnCorrectedReference, reference keyframe, expected vertex)
    for m, r in enumerate(s["point_ref"]):
        if r < 0:
            away = (bad_kf, out_kf)[m % 2]
            pts.append((0, s["Xw"][m], 0, 0, away, -1) if m % 4 < 2 else (0, s["Xw"][m], ids[cur], ids[away], K(0), -1))
        elif m % 2:
            pts.append((0, s["Xw"][m], ids[cur], ids[K(r)], K((r + 1) % n), vertex_of.get(K(r), -1)))
        else:
            pts.append((0, s["Xw"][m], 7, ids[K((r + 1) % n)], K(r), vertex_of.get(K(r), -1)))
    pts.insert(2, (1, F32([1, 2, 3]), 0, 0, K(1), -1))
    if all_bad:
        pts = [(1,) + p[1:] for p in pts]
    blob = [n_all, len(pts), n_iterations, s["fix_scale"], loop, cur, 0, 0, len(LC)] + [0] * 7
    sv = {kf_of_vertex[v]: v for v in range(n)}
    for k in range(n_all):
        T = s["Tcw"][sv[k]] if k in sv else np.eye(4, dtype=F32)[:3].reshape(-1)
        blob += [ids[k], float(bad[k]), float(in_map[k]), parent[k], *T, len(loops[k]), len(by_weight[k]), len(children[k])]
        blob += sorted(loops[k])
        for o in by_weight[k]:
            blob += [o, cov[k][o]]
        blob += sorted(children[k])
    tables = []
    for flag, rows in (("has_noncorrected", "Snoncorrected"), ("has_corrected", "Scorrected")):
        entries = [(K(v), s[rows][v]) for v in range(n) if s[flag][v]] + [(out_kf, np.array([0, 0, 0, 1, 1, 2, 3, 1.5]))]
        tables.append(len(entries))
        for k, row in entries:
            blob += [k, *row]
    blob[6], blob[7] = tables
    for key in sorted(LC):
        blob += [key, len(LC[key]), *sorted(LC[key])]
    for p in pts:
        blob += [p[0], *p[1], p[2], p[3], p[4]]
    order = [sv[k] for k in good]
    live = [p for p in pts if not p[0]]
    problem = dict(Tcw=s["Tcw"][order], has_corrected=s["has_corrected"][order], Scorrected=s["Scorrected"][order],
                   has_noncorrected=s["has_noncorrected"][order], Snoncorrected=s["Snoncorrected"][order],
                   fixed=np.array([k == loop for k in good], np.uint8),
                   edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
                   edge_kind=np.array([e[2] for e in edges], np.uint8),
                   Xw=np.array([p[1] for p in live], F32).reshape(-1, 3), point_ref=np.array([p[5] for p in live], np.int32),
                   fix_scale=s["fix_scale"])
    written = [m for m, p in enumerate(pts) if not p[0]]
    return np.array(blob, np.float64), problem, good, written


def _run_adapter(exe, tmp_path, blob):
    (tmp_path / "scene.bin").write_bytes(np.asarray(blob, np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path / "scene.bin"), str(tmp_path / "out.txt")], check=True, timeout=120)
    return [line.split() for line in (tmp_path / "out.txt").read_text().split("\n") if line]


ADAPTER = {"tables": 16, "f7": 11}  # fixture: seed of the world around it (bFixScale false, true)
ADAPTER_ITERATIONS = 2


@functools.lru_cache(maxsize=None)
def _adapter_case(name):
    blob, problem, good, written = _adapter_world(scene(name), np.random.default_rng(ADAPTER[name]), ADAPTER_ITERATIONS)
    return blob, problem, good, written, er.run_scene(problem, ADAPTER_ITERATIONS)


@pytest.mark.parametrize("name", list(ADAPTER))
def test_adapter_world_exercises_every_filter(name):
    """the enumeration keeps and drops what it should on the stand-in world, and the restatement's run on
    it is decisive"""
    blob, problem, good, written, r = _adapter_case(name)
    kinds = problem["edge_kind"]
    n = len(good)
    assert n == len(scene(name)["Tcw"]) and (kinds == 0).sum() == 3 and (kinds == 1).sum() >= n - 1 + 2
    pairs = {(min(i, j), max(i, j)) for i, j in zip(problem["edge_i"], problem["edge_j"])}
    assert len(pairs) == len(kinds)  # no pair twice: the parent, child, loop-edge and sInsertedEdges filters
    assert r.iterations == ADAPTER_ITERATIONS and r.n_free == n - 1 and er.decisive(r), min(r.trace.margins + r.fn.margins)
    assert (problem["point_ref"] < 0).sum() >= 1 and (problem["point_ref"] >= 0).sum() >= 4


def test_adapter_builds_and_with_nothing_that_is_not_bad_touches_nothing(essential_main, tmp_path):
    """EssentialGraphOptimizer.h compiles against the stand-ins with -Wall -Wextra -Werror; when every
    keyframe and MapPoint is bad there is no vertex: no device is needed and nothing is written"""
    blob, *_ = _adapter_world(scene("tables"), np.random.default_rng(5), 2, all_bad=True)
    lines = _run_adapter(essential_main, tmp_path, blob)
    assert lines == [["F", "1"]]


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


def run_device(s, n_iterations, stream=None, workspace=None, mutate=None):
    """the device form on guarded copies, outputs and workspace pre-filled with 0x5A; returns (record,
    Scw_out (N, 8), Tcw_out (N, 16), Xw_out (M, 3), workspace tensor triple); checks the guards and that no
    input changed"""
    torch = _torch_gpu()
    a = essential.pack(*(s[k] for k in er.ARRAYS))
    if mutate:
        mutate(a)
    tn, te, tm = len(a["Tcw"]), len(a["edge_i"]), len(a["Xw"])
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d_in = [_guarded(torch, a[n]) for n, *_ in essential.INPUTS]
        d_S = _guarded(torch, np.zeros((tn, 8), np.float64), 0x5A)
        d_T = _guarded(torch, np.zeros((tn, 16), F32), 0x5A)
        d_X = _guarded(torch, np.zeros((tm, 3), F32), 0x5A)
        ws = workspace or _guarded(torch, np.zeros(essential.workspace_bytes(tn, te, tm), np.uint8), 0x5A)
        before = [f.clone() for f, *_ in d_in]
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    res = essential.optimize_essential_graph_device(*(v for _, v, _ in d_in), s["fix_scale"], n_iterations, d_S[1],
                                                    d_T[1], d_X[1], ws[1], stream=stream)
    torch.cuda.synchronize()
    for (f, *_), b in zip(d_in, before):
        assert torch.equal(f, b)
    _guards_intact(d_in + [d_S, d_T, d_X, ws])
    return res, d_S[1].cpu().numpy(), d_T[1].cpu().numpy(), d_X[1].cpu().numpy(), ws


def check_against_ref(res, S, T, X, r, s, label):
    assert er.decisive(r), label  # the condition on the inputs
    dev = deviation(S, T, X, r)
    print(f"{label}: deviation {dev:.3f} ulp (bound {ULP_BOUND:.3f}), iterations {res['iterations']} rejected "
          f"{res['rejected']} n_free {res['n_free']} active edges {res['n_active_edges']}; restatement {r.iterations} "
          f"{r.rejected} {r.n_free} {r.n_active_edges}; chi2 {res['first_chi2']:.6g} -> {res['last_chi2']:.6g} "
          f"({r.first_chi:.6g} -> {r.last_chi:.6g})")
    assert res["status"] == 0 and T.shape == (len(r.Tcw), 16) and X.shape == r.Xw.shape and S.shape == r.Scw.shape
    assert tuple(int(res[c]) for c in COUNTERS) == tuple(getattr(r, c) for c in COUNTERS), label
    assert dev <= ULP_BOUND, (label, dev)
    assert np.array_equal(T[:, 12:], np.tile(F32([0, 0, 0, 1]), (len(T), 1))), label
    if s["fix_scale"]:
        assert S[:, 7].tobytes() == r.Scw[:, 7].tobytes() == np.asarray(r.job.vScw[7]).tobytes(), label
    keep = s["point_ref"] < 0
    assert X[keep].tobytes() == s["Xw"][keep].tobytes(), label
    # the sums are added in one order on both sides; what differs is the five functions, magnified by the
    # 1e-9 differences into 1e-6 of a step: 1e-9 of the first chi2 (no step yet), 1e-6 of the chi2 the run
    # started from for the last (the decisions stay 1e-6 of a chi2 away), 1e-4 of lambda (globalba's)
    for got, want, tol in ((res["first_chi2"], r.first_chi, 1e-9 * abs(r.first_chi)),
                           (res["last_chi2"], r.last_chi, 1e-6 * abs(r.first_chi)),
                           (res["last_lambda"], r.last_lambda, 1e-4 * abs(r.last_lambda))):
        assert abs(got - want) <= tol, (label, got, want)
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_gpu_fixture(name):
    """every fixture through the device form; the host form gives the same bytes"""
    s, r, it = scene(name), ref(name), FIXTURES[name][1]
    res, S, T, X, _ = run_device(s, it)
    check_against_ref(res, S, T, X, r, s, name)
    S1, T1, X1, res1 = essential.optimize_essential_graph(*(s[k] for k in er.ARRAYS), s["fix_scale"], it)
    assert S1.tobytes() == S.tobytes() and T1.tobytes() == T.tobytes() and X1.tobytes() == X.tobytes()
    assert res1.tobytes() == res.tobytes()


@pytest.mark.gpu
def test_gpu_zero_iterations_write_the_round_trip():
    s, r = scene("f7"), ref("f7", 0)
    res, S, T, X, _ = run_device(s, 0)
    assert S.tobytes() == r.Scw.tobytes() and T.reshape(-1, 4, 4).tobytes() == r.Tcw.tobytes()
    assert X.tobytes() == r.Xw.tobytes()
    assert (int(res["iterations"]), int(res["rejected"])) == (0, 0) and res["n_free"] == r.n_free == 7
    assert res["n_active_edges"] == r.n_active_edges


@pytest.mark.gpu
def test_gpu_determinism_and_a_used_workspace():
    """two calls give equal bytes, the second on the workspace the first left"""
    s, it = scene("f16"), FIXTURES["f16"][1]
    res, S, T, X, ws = run_device(s, it)
    res2, S2, T2, X2, _ = run_device(s, it, workspace=ws)
    assert res.tobytes() == res2.tobytes() and S.tobytes() == S2.tobytes() and T.tobytes() == T2.tobytes()
    assert X.tobytes() == X2.tobytes()
    s, it = scene("far"), FIXTURES["far"][1]
    a, b = run_device(s, it), run_device(s, it)
    assert all(a[k].tobytes() == b[k].tobytes() for k in range(4))


@pytest.mark.gpu
def test_gpu_device_form_on_a_stream():
    torch = _torch_gpu()
    s, it = scene("f14"), FIXTURES["f14"][1]
    res, S, T, X, _ = run_device(s, it, stream=torch.cuda.Stream())
    check_against_ref(res, S, T, X, ref("f14"), s, "f14 on a stream")


@pytest.mark.gpu
def test_gpu_nan_pose_ends_inside_the_loop_bound():
    """a NaN in a free keyframe's pose: every trial is rejected, the call returns within n_iterations
    (1 + 10) passes, and a keyframe no edge joins to it keeps its round trip"""
    it = FIXTURES["gap"][1]
    s = scene("gap", nan_pose=2)
    res, S, T, X, _ = run_device(s, it)
    trials = int(res["rejected"])
    print(f"NaN pose: iterations {res['iterations']}, rejected {trials}")
    assert res["status"] == 0 and 1 <= res["iterations"] <= it and res["iterations"] <= trials <= 10 * it
    rt = round_trip(s)
    for v in (0, 4):
        assert S[v].tobytes() == rt.Scw[v].tobytes() and T[v].tobytes() == rt.Tcw[v].tobytes()


@pytest.mark.gpu
def test_gpu_bad_index_is_rejected_and_nothing_is_written():
    s = scene("e65")
    for key, at, value in (("edge_i", 40, 10), ("edge_i", 0, -1), ("edge_j", 64, 10), ("edge_j", 30, -3),
                           ("edge_j", 7, None), ("point_ref", 3, 10)):
        def mutate(a, key=key, at=at, value=value):
            a[key] = a[key].copy()
            a[key][at] = a["edge_i"][at] if value is None else value  # None: i == j
        res, S, T, X, _ = run_device(s, 3, mutate=mutate)
        assert res["status"] == -1 and res["iterations"] == 0, (key, at)
        assert all((o.view(np.uint8) == 0x5A).all() for o in (S, T, X)), (key, at)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ADAPTER))
def test_gpu_adapter(essential_main, tmp_path, name):
    """OptimizeEssentialGraphGPU on stand-in keyframes, MapPoints, Map and Sim3, bFixScale false and
    true: the edge list, the tables' flags, the fixed vertex and the points' references it hands to the
    library against the Python enumeration of the same world; every SetPose, SetWorldPos and
    UpdateNormalAndDepth in order, under mMutexMapUpdate, with the values of the restatement run on that
    problem"""
    _torch_gpu()
    blob, problem, good, written, r = _adapter_case(name)
    assert er.decisive(r) and r.iterations >= 1
    lines = _run_adapter(essential_main, tmp_path, blob)
    hexf = lambda words: np.array([int(w, 16) for w in words], np.uint32).view(F32)
    by = lambda tag: [l[1:] for l in lines if l[0] == tag]
    n, E, M = len(good), len(problem["edge_i"]), len(written)
    assert by("N") == [[str(n), str(E), str(M), str(problem["fix_scale"]), str(ADAPTER_ITERATIONS)]]
    assert [tuple(int(v) for v in e) for e in by("E")] == list(zip(problem["edge_i"].tolist(), problem["edge_j"].tolist(),
                                                                   problem["edge_kind"].tolist()))
    assert [[int(v) for v in row[1:]] for row in by("V")] == [
        [int(problem["has_corrected"][v]), int(problem["has_noncorrected"][v]), int(problem["fixed"][v])] for v in range(n)]
    assert [int(row[1]) for row in by("R")] == problem["point_ref"].tolist()
    calls = [l for l in lines if l[0] in "LPWUF"]
    assert [l[0] for l in calls] == ["L"] + ["P"] * n + ["W", "U"] * M + ["F"]
    assert calls[0] == ["L", "1"] and calls[-1] == ["F", "1"]  # held during the write-back, released after
    assert [int(l[1]) for l in calls[1:1 + n]] == good
    assert [int(l[1]) for l in calls[1 + n:-1:2]] == written == [int(l[1]) for l in calls[2 + n:-1:2]]
    T = np.stack([hexf(l[2:]) for l in calls[1:1 + n]])
    X = np.stack([hexf(l[2:]) for l in calls[1 + n:-1:2]])
    dev = max(_ulps(T.reshape(-1, 4, 4), r.Tcw), _ulps(X, r.Xw))
    print(f"adapter {name}: deviation {dev:.3f} ulp, iterations {r.iterations}, {E} edges")
    assert dev <= ULP_BOUND
    keep = problem["point_ref"] < 0
    assert X[keep].tobytes() == problem["Xw"][keep].tobytes()
