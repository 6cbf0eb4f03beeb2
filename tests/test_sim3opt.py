"""Sim3 refinement (include/orbgpu_sim3opt.h, csrc/sim3opt.hip,
include/orbslam2_amd/Sim3Optimizer.h) against the numpy restatement of
Optimizer::OptimizeSim3 (tests/sim3opt_ref.py).

Parity: every element of the float32 T12 within ULP_BOUND float32 ulps at the
scale max(1, max|T12|); flags, n_in, rounds and n_bad_first equal.  g2o's 1e-9
central differences make the Jacobian a noisy function of the estimate's last
bits, so the converged estimate depends on the order in which the edges are
summed; the kernel and the restatement differ in exactly that.  The bound is
therefore measured, not fixed: MEASURED_WORST is the largest deviation of T12
the restatement shows on any fixture below when its correspondences are
permuted (8 permutations each), and ULP_BOUND = max(2, 4 x MEASURED_WORST) --
the factor 4 because the maximum of a few samples of a noise distribution
underestimates its tail, the floor 2 as in test_poseopt.py (one ulp for a
double on a float rounding boundary, one of slack).
test_ref_permutation_spread_of_every_fixture asserts the measurement.  The LM
traces are not compared (at convergence accept / reject is decided by rounding
noise): lm_iterations is only checked for its range.  Every scene's seed is
fixed and, in the restatement, keeps every chi2 either check reads at least
1e-6 (relative) away from th2; the tests assert that on the CPU before they
compare.
"""
import ctypes
import functools
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orbgpu
import sim3opt
import sim3opt_ref
import synth

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
ULP = 2.0 ** -23
MARGIN = 1e-6
# the restatement's worst T12 deviation under 8 permutations of any fixture (the far start, seed
# 117: 0.8563 ulp, rounded up; n = 256: 0.835; all others <= 0.5), measured on the CPU
MEASURED_WORST = 0.857
ULP_BOUND = max(2.0, 4.0 * MEASURED_WORST)  # 3.428
PERMUTATIONS = 8
KEYS = tuple(name for name, _ in sim3opt.ARRAYS)
CAP = 768  # csrc/sim3opt.hip: correspondences of a job kept in LDS

CLEAN = dict(outliers=0.0, noise=0.5)
# n of the size sweep -> scene: the n == 0 and survivors < 10 rules (0, 1, 9 with outliers; 10 and
# 11 without, so exactly 10 survivors still run the second optimisation), the wave (64) and
# workgroup (256) boundaries, more than one correspondence per lane, and CAP + 3: read from HBM
SIZES = {0: dict(seed=100), 1: dict(seed=101), 9: dict(seed=109), 10: dict(seed=110, **CLEAN),
         11: dict(seed=111, **CLEAN), 63: dict(seed=163), 64: dict(seed=164), 65: dict(seed=165),
         255: dict(seed=355), 256: dict(seed=356), 257: dict(seed=357), CAP + 3: dict(seed=871)}
# `far`: a start 0.3 rad / 0.5 m / 30 % in scale off whose trace in the restatement has a rejected
# trial followed by an accepted one that lowers the robust chi2 by more than 1 % (seeds searched on
# the CPU from 61 upwards); `few`: half of 14 correspondences are outliers, fewer than 10 survive
CASES = {
    "fix_on": dict(n=300, seed=11, fix_scale=True),
    "fix_off": dict(n=300, seed=21),
    "clean": dict(n=120, seed=31, **CLEAN),
    "far": dict(n=300, seed=117, start_rot=0.3, start_t=0.5, start_s=1.3),
    "few": dict(n=14, seed=41, outliers=0.5),
    "behind": dict(n=65, seed=51, behind=1),
}


@functools.lru_cache(maxsize=None)
def _scene_cached(items):
    kw = dict(items)
    s = synth.sim3opt_scene(kw.pop("n"), kw.pop("seed"), **kw)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def scene(**kw):
    return _scene_cached(tuple(sorted(kw.items())))


def run_ref(s, perm=None):
    a = [s[k] if perm is None else s[k][perm] for k in KEYS]
    return sim3opt_ref.optimize_sim3(s["q12"], s["t12"], s["s12"], *a, s["K1"], s["K2"], s["th2"], s["fix_scale"])


@functools.lru_cache(maxsize=None)
def _ref_cached(items):
    return run_ref(_scene_cached(items))


def ref(**kw):
    """the restatement's result of a scene, computed once per session, with the margin precondition"""
    r = _ref_cached(tuple(sorted(kw.items())))
    assert sim3opt_ref.threshold_margin(r, scene(**kw)["th2"]) >= MARGIN, kw
    return r


def size_scene(n):
    return dict(n=n, **SIZES[n])


def all_fixtures():
    return [(f"n={n}", size_scene(n)) for n in SIZES] + list(CASES.items())


def job_tuple(s, offset):
    return (len(s["P1c"]), offset, s["q12"], s["t12"], s["s12"], s["K1"], s["K2"], s["th2"], s["fix_scale"])


def pack(scenes):
    """(jobs, the six arrays) of a list of scenes laid out back to back"""
    cands, off = [], 0
    for s in scenes:
        cands.append(job_tuple(s, off))
        off += len(s["P1c"])
    arrays = [np.concatenate([s[k].reshape(-1, w) for s in scenes]) if scenes else np.zeros((0, w), F32)
              for k, w in sim3opt.ARRAYS]
    arrays[4], arrays[5] = arrays[4].reshape(-1), arrays[5].reshape(-1)
    return sim3opt.make_jobs(cands), arrays


def t12_deviation(a, b):
    """largest element difference of two float32 T12 in float32 ulps at the scale max(1, max|b|)"""
    scale = max(1.0, float(np.abs(b).max()))
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / (ULP * scale)


def input_bytes(s):
    return np.array([*s["q12"], *s["t12"], s["s12"]], np.float64).tobytes()


def check_against_ref(res, flags, r, s, label):
    """one job's RESULT_DTYPE record and flag bytes against the restatement; returns the deviation in ulps"""
    T = res["T12"].reshape(4, 4)
    dev = t12_deviation(T, r.T12)
    print(f"{label}: T12 deviation {dev:.3f} ulp (bound {ULP_BOUND:.3f}), n_in {res['n_in']}, rounds {res['rounds']}, "
          f"n_bad_first {res['n_bad_first']}, iterations {list(res['lm_iterations'])}, rejected "
          f"{list(res['lm_rejected'])}; restatement {[(t.iterations, t.rejected) for t in r.trace]}")
    assert np.array_equal(flags.astype(bool), r.removed), (label, int((flags.astype(bool) != r.removed).sum()))
    assert set(np.unique(flags)) <= {0, 1}, label
    assert (int(res["n_in"]), int(res["rounds"]), int(res["n_bad_first"])) == (r.n_in, r.rounds, r.n_bad_first), label
    assert dev <= ULP_BOUND, (label, dev)
    # float(q12, t12, s12) is consistent with T12: the same expression on the returned doubles
    S = (list(res["q12"]), list(res["t12"]), float(res["s12"]))
    assert sim3opt_ref.sim3_to_T(S).tobytes() == T.tobytes(), label
    got = np.array([*res["q12"], *res["t12"], res["s12"]], np.float64).tobytes()
    if r.rounds < 2:
        assert got == input_bytes(s), label  # g2oS12 is not written
    if s["fix_scale"]:
        assert np.float64(res["s12"]).tobytes() == np.float64(s["s12"]).tobytes(), label
    limits = (5, 10)
    for k in range(2):
        if k < r.rounds:
            assert 1 <= res["lm_iterations"][k] <= limits[k] and 0 <= res["lm_rejected"][k] <= 100, label
        else:
            assert res["lm_iterations"][k] == 0 and res["lm_rejected"][k] == 0, label
    return dev


# ---------------------------------------------------------------- CPU: the restatement's own checks

def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _analytic_jacobians(S, p):
    """d e / d u at u = 0 of both edges for the update Sim3(u) * S: e12 = obs1 - cam1(S P2), e21 =
    obs2 - cam2(S^-1 P1).  With p = S P2: d p / d u = [-[p]x | I | p]; with p = S^-1 P1 =
    R^T (P1 - t) / s: d p / d u = R^T [[P1]x | -I | -P1] / s."""
    q, t, s = S
    R = np.array(sim3opt_ref.quat_to_R(q))
    out = []
    for edge in (0, 1):
        K = p.K2 if edge else p.K1
        J = np.zeros((p.n, 2, 7))
        for i in range(p.n):
            if edge == 0:
                pt = s * (R @ p.P2[i]) + np.array(t)
                dp = np.hstack([-_skew(pt), np.eye(3), pt[:, None]])
            else:
                pt = R.T @ (p.P1[i] - np.array(t)) / s
                dp = R.T @ np.hstack([_skew(p.P1[i]), -np.eye(3), -p.P1[i][:, None]]) / s
            x, y, z = pt
            dproj = np.array([[K[0] / z, 0, -K[0] * x / z ** 2], [0, K[1] / z, -K[1] * y / z ** 2]])
            J[i] = -dproj @ dp
        out.append(J)
    return out


def test_ref_numeric_jacobian_agrees_with_the_analytic_derivative():
    """Column d of the numeric Jacobian is (e(+delta) - e(-delta)) / (2 delta) with delta = 1e-9.
    Its truncation error, O(delta^2), is nothing; its noise is the rounding of the two errors.  An
    error is obs - (f x / z + c): the last subtraction alone rounds a value of magnitude M =
    max(|obs|, |f x / z + c|) to M eps / 2, and the chain before it (the quaternion product of the
    update, the rotation, s r + t, the quotient, f v + c) rounds C operations of relative error
    eps / 2 each on quantities whose effect on the pixel is at most f (|p| + |t|) / |z| -- a
    perturbation eps |p| of the mapped point moves the projection by f eps |p| / z.  Two errors,
    divided by 2 delta: |J_num - J_ana| <= C eps (M + f (|p| + |t|) / |z|) / (2 delta), with C = 32
    for the about thirty rounded operations between the update vector and the error."""
    eps = 2.0 ** -52
    C = 32
    for seed, fix in ((71, False), (72, True)):
        s = synth.sim3opt_scene(40, seed, fix_scale=fix)
        p = sim3opt_ref.problem(*(s[k] for k in KEYS), s["K1"], s["K2"])
        S = (list(s["q12"]), list(s["t12"]), s["s12"])
        J12, J21 = sim3opt_ref.numeric_jacobians(S, p, fix)
        A12, A21 = _analytic_jacobians(S, p)
        Sinv = sim3opt_ref.sim3_inverse(S)
        worst = 0.0
        for Jn, Ja, St, P, obs, K in ((J12, A12, S, p.P2, p.o1, p.K1), (J21, A21, Sinv, p.P1, p.o2, p.K2)):
            x, y, z = sim3opt_ref.sim3_map(St, (P[:, 0], P[:, 1], P[:, 2]))
            uv = np.stack([(x / z) * K[0] + K[2], (y / z) * K[1] + K[3]], 1)
            M = np.maximum(np.abs(obs), np.abs(uv)).max(1)
            reach = max(K[0], K[1]) * (np.sqrt(x * x + y * y + z * z) + np.linalg.norm(St[1])) / np.abs(z)
            bound = C * eps * (M + reach) / (2 * sim3opt_ref.DELTA)
            for d in range(7):
                num = np.stack(Jn[d], 1)
                ana = Ja[:, :, d]
                if fix and d == 6:
                    assert (num == 0).all()  # exactly zero: Sim3(0) is the exact identity
                    continue
                err = np.abs(num - ana).max(1)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (seed, d, float((err / bound).max()))
            assert np.abs(Ja).max() > 10  # the derivative is hundreds of pixels per unit: the bound (~1e-2) is tight
        print(f"seed {seed}: largest |J_num - J_ana| / bound = {worst:.3f}")


def test_ref_exp_returns_a_rotation_on_both_sides_of_each_branch():
    rng = np.random.default_rng(6)
    for th in (1e-7, 0.99e-5, 1.01e-5, 1e-3, 0.3, 2.5):
        for sigma in (0.0, 1e-9, 0.99e-5, -0.99e-5, 1.01e-5, -1.01e-5, 0.2, -0.4):
            axis = rng.normal(size=3)
            om = axis / np.linalg.norm(axis) * th
            up = rng.normal(size=3)
            q, t, s = sim3opt_ref.sim3_exp([*om, *up, sigma])
            R = np.array(sim3opt_ref.quat_to_R(q))
            # the small-angle branch is I + O + O^2, a rotation to O(theta^2): 1e-10 at theta = 1e-5
            tol = 1e-9 if th < 1e-5 else 1e-12
            assert np.abs(R @ R.T - np.eye(3)).max() < tol and abs(np.linalg.det(R) - 1) < tol, (th, sigma)
            assert abs(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)) - th) < 1e-6
            assert s == math.exp(sigma)
            # t = W upsilon with W = C I + O(theta): within theta |upsilon| (and sigma) of upsilon.  Not
            # in the branch |sigma| >= 1e-5, theta < 1e-5: the reference's B there, ((sigma^2 / 2 - sigma
            # + 1) s) / sigma^3, lacks the "- 1" of the series and is about 1 / sigma^3, so B Omega^2 is
            # not small (sim3.h:116); it is restated as written.
            if not (abs(sigma) >= 1e-5 and th < 1e-5):
                assert np.abs(np.array(t) - up).max() <= (2 * th + 2 * abs(sigma)) * np.linalg.norm(up) + 1e-15
    q, t, s = sim3opt_ref.sim3_exp([0.0] * 7)
    assert q == [0.0, 0.0, 0.0, 1.0] and t == [0.0, 0.0, 0.0] and s == 1.0
    # above theta = 1e-5 the branches meet across sigma = 1e-5 up to the small-sigma branch's own
    # approximation (C = 1 for (s - 1) / sigma = 1 + sigma / 2: 5e-6 relative)
    up = [0.3, -0.2, 0.5]
    for om in ([1.01e-5, 0, 0], [0.2, 0.1, -0.3]):
        a = sim3opt_ref.sim3_exp([*om, *up, 0.99e-5])
        b = sim3opt_ref.sim3_exp([*om, *up, 1.01e-5])
        assert np.abs(np.array(a[1]) - np.array(b[1])).max() < 2 * 1e-5 * np.linalg.norm(up)


def test_ref_fix_scale_keeps_the_scale_bits_and_a_zero_seventh_column():
    s = scene(**CASES["fix_on"])
    p = sim3opt_ref.problem(*(s[k] for k in KEYS), s["K1"], s["K2"])
    S = (list(s["q12"]), list(s["t12"]), s["s12"])
    for fix, zero in ((True, True), (False, False)):
        J12, J21 = sim3opt_ref.numeric_jacobians(S, p, fix)
        for J in (J12, J21):
            assert all((c == 0).all() for c in J[6]) == zero
            assert all(any((c != 0).any() for c in J[d]) for d in range(6))
    r = ref(**CASES["fix_on"])
    assert r.rounds == 2 and np.float64(r.S[2]).tobytes() == np.float64(s["s12"]).tobytes()
    assert r.S[0] != list(s["q12"]) and r.S[1] != list(s["t12"])
    r = ref(**CASES["fix_off"])
    assert r.rounds == 2 and r.S[2] != scene(**CASES["fix_off"])["s12"]


def test_ref_noise_free_flags_exactly_the_injected_outliers():
    for seed, n, fix in ((81, 120, False), (82, 300, True)):
        s = synth.sim3opt_scene(n, seed, noise=0.0, outliers=0.2, fix_scale=fix)
        r = run_ref(s)
        assert s["outlier"].sum() > 10 and np.array_equal(r.removed, s["outlier"])
        assert r.n_in == n - s["outlier"].sum() and r.rounds == 2 and r.n_bad_first == s["outlier"].sum()
        p = sim3opt_ref.take(sim3opt_ref.problem(*(s[k] for k in KEYS), s["K1"], s["K2"]), ~s["outlier"])

        def cost(S):
            _, _, c12, c21 = sim3opt_ref.edge_errors(S, p)
            return c12.sum() + c21.sum()
        assert cost(r.S) < 1e-3 * cost((list(s["q12"]), list(s["t12"]), s["s12"]))
        R_est = np.array(sim3opt_ref.quat_to_R(r.S[0]))
        assert np.abs(R_est - s["R_true"]).max() < 1e-4 and np.abs(np.array(r.S[1]) - s["t_true"]).max() < 1e-3
        assert abs(r.S[2] - s["s_true"]) < 1e-3


def test_ref_rules_for_few_correspondences():
    s = scene(**size_scene(0))
    r = ref(**size_scene(0))
    assert (r.n_in, r.rounds, r.n_bad_first, len(r.trace)) == (0, 0, 0, 0) and r.S[2] is not None
    assert np.array([*r.S[0], *r.S[1], r.S[2]]).tobytes() == input_bytes(s)
    # fewer than 10 survivors: 0 returned, S untouched, the first check's flags kept
    s, r = scene(**CASES["few"]), ref(**CASES["few"])
    assert r.rounds == 1 and r.n_in == 0 and 0 < r.n_bad_first == r.removed.sum() and 14 - r.n_bad_first < 10
    assert np.array([*r.S[0], *r.S[1], r.S[2]]).tobytes() == input_bytes(s)
    assert r.T12.tobytes() == sim3opt_ref.sim3_to_T((list(s["q12"]), list(s["t12"]), s["s12"])).tobytes()
    for n in (1, 9):
        assert ref(**size_scene(n)).rounds == 1 and ref(**size_scene(n)).n_in == 0
    # exactly 10 survivors run the second optimisation
    r = ref(**size_scene(10))
    assert r.rounds == 2 and r.n_bad_first == 0 and r.n_in == 10

    # no outliers: 5 more iterations; outliers: 10.  Counted by wrapping optimize().
    calls = []
    inner = sim3opt_ref.optimize

    def spy(est, p, iterations, *a):
        calls.append((p.n, iterations))
        return inner(est, p, iterations, *a)
    sim3opt_ref.optimize = spy
    try:
        r = run_ref(scene(**CASES["clean"]))
        assert r.n_bad_first == 0 and calls == [(120, 5), (120, 5)]
        calls.clear()
        r = run_ref(scene(**CASES["fix_off"]))
        assert r.n_bad_first > 0 and calls == [(300, 5), (300 - r.n_bad_first, 10)]
    finally:
        sim3opt_ref.optimize = inner


@pytest.mark.parametrize("label,kw", all_fixtures(), ids=[label for label, _ in all_fixtures()])
def test_ref_permutation_spread_of_every_fixture(label, kw):
    """the same scene with its correspondences permuted (every sum rounds differently), 8 times:
    T12 within a quarter of the GPU tests' bound of the unpermuted result -- the measurement
    ULP_BOUND is made from -- with flags, return value and round counts equal"""
    s, a = scene(**kw), ref(**kw)
    n = len(s["P1c"])
    worst = 0.0
    for k in range(PERMUTATIONS):
        p = np.random.default_rng(1000 + k).permutation(n)
        b = run_ref(s, p)
        assert sim3opt_ref.threshold_margin(b, s["th2"]) >= MARGIN
        assert np.array_equal(a.removed[p], b.removed)
        assert (a.n_in, a.rounds, a.n_bad_first) == (b.n_in, b.rounds, b.n_bad_first)
        worst = max(worst, t12_deviation(b.T12, a.T12))
    print(f"{label}: permutation spread {worst:.3f} ulp")
    assert worst <= ULP_BOUND / 4
    assert worst <= MEASURED_WORST + 1e-3


def test_scene_preconditions():
    """every fixed scene keeps the chi2 both checks read away from th2; the far-start fixture's
    trace has a rejected trial followed by an accepted one before convergence; the behind-the-
    camera scene has its point behind keyframe 1 (z < 0, not 0) at the start and at the end"""
    for label, kw in all_fixtures():
        ref(**kw)
    for n in SIZES:
        assert ref(**size_scene(n)).rounds == (0 if n == 0 else 1 if n < 10 else 2), n
    for name in ("fix_on", "fix_off", "far", "behind"):
        r = ref(**CASES[name])
        assert r.rounds == 2 and 0 < r.n_bad_first and 0 < r.n_in < CASES[name]["n"], name
    assert ref(**CASES["clean"]).n_bad_first == 0 and ref(**CASES["clean"]).rounds == 2
    found = False
    for tr in ref(**CASES["far"]).trace:
        for k in range(1, len(tr.trials)):
            if not tr.trials[k - 1] and tr.trials[k] and tr.chi_after[k] < 0.99 * tr.chi_after[k - 1]:
                found = True
    assert found
    s, r = scene(**CASES["behind"]), ref(**CASES["behind"])
    for S in ((list(s["q12"]), list(s["t12"]), s["s12"]), r.S):
        P2 = s["P2c"].astype(np.float64)
        z = sim3opt_ref.sim3_map(S, (P2[:, 0], P2[:, 1], P2[:, 2]))[2]
        assert z[0] < 0 and (z[1:] > 0).all()
    assert r.removed[0]


# ---------------------------------------------------------------- CPU: argument checks of the library

def _jobs2(n0=4, off0=0, n1=6, off1=4):
    q, t, K = (0, 0, 0, 1), (0, 0, 0), (500, 500, 320, 240)
    return sim3opt.make_jobs([(n0, off0, q, t, 1.0, K, K, 10.0, False), (n1, off1, q, t, 1.0, K, K, 10.0, True)])


ARRAY_ARGS = ("P1c", "P2c", "obs1", "obs2", "w1", "w2")


def _args(form, **kw):
    a = dict(batch=2, jobs=_jobs2(), total=10, res=1 << 15, out=1 << 16)
    a.update({name: 1 << (12 + k) for k, name in enumerate(ARRAY_ARGS)})
    a["res"], a["out"] = 1 << 20, 1 << 21
    a.update(kw)
    jobs = a["jobs"]
    jp = None if jobs is None else (jobs.ctypes.data if form == "host" else 1 << 22)
    L = orbgpu.lib()
    arrays = [a[name] for name in ARRAY_ARGS]
    if form == "host":
        return L.orbgpu_optimize_sim3_batch(a["batch"], jp, a["total"], *arrays, a["res"], a["out"])
    return L.orbgpu_optimize_sim3_batch_device(a["batch"], jp, a["total"], *arrays, a["res"], a["out"], None)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_checks_need_no_device(form):
    """rejected on the host before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    assert _args(form, batch=-1) == E and _args(form, total=-1) == E
    for name in ("jobs", *ARRAY_ARGS, "res", "out"):
        assert _args(form, **{name: None}) == E, name
    assert "null" in orbgpu.last_error()
    assert _args(form, batch=0) == orbgpu.OK
    none = {name: None for name in ARRAY_ARGS}
    assert _args(form, batch=0, total=0, jobs=None, res=None, out=None, **none) == orbgpu.OK


def test_job_range_checks_need_no_device():
    E = orbgpu.ERR_ARG
    assert _args("host", jobs=_jobs2(-1, 0)) == E
    assert "job 0" in orbgpu.last_error()
    assert _args("host", jobs=_jobs2(4, -1)) == E
    assert _args("host", jobs=_jobs2(4, 0, 7, 4)) == E  # 4 + 7 > 10
    assert "job 1" in orbgpu.last_error()
    assert _args("host", jobs=_jobs2(4, 0, 1, 10)) == E
    assert _args("host", jobs=_jobs2(4, 0, 2 ** 31 - 1, 2 ** 31 - 1)) == E  # the sum does not wrap
    # total_corr == 0: every job is empty; the host writes the results, nothing is launched
    j = _jobs2(0, 0, 0, 0)
    j["q12"][1], j["t12"][1], j["s12"][1] = (0.1, -0.2, 0.3, 0.9), (1.5, -2.5, 3.5), 1.25
    res = np.full(2 * sim3opt.RESULT_DTYPE.itemsize, 0x5A, np.uint8).view(sim3opt.RESULT_DTYPE)
    none = {name: None for name in ARRAY_ARGS}
    assert _args("host", jobs=j, total=0, out=None, res=res.ctypes.data, **none) == orbgpu.OK
    assert res["n_in"].tolist() == [0, 0] and res["rounds"].tolist() == [0, 0] and res["n_bad_first"].tolist() == [0, 0]
    assert not res["lm_iterations"].any() and not res["lm_rejected"].any()
    for k in range(2):
        got = np.array([*res["q12"][k], *res["t12"][k], res["s12"][k]]).tobytes()
        assert got == np.array([*j["q12"][k], *j["t12"][k], j["s12"][k]]).tobytes()
        S = (list(j["q12"][k]), list(j["t12"][k]), float(j["s12"][k]))
        assert res["T12"][k].tobytes() == sim3opt_ref.sim3_to_T(S).tobytes()
    assert res["T12"][0].tolist() == np.eye(4).reshape(-1).tolist()
    assert _args("host", jobs=_jobs2(1, 0, 0, 0), total=0, out=None, **none) == E


def _header_struct(name):
    """(size, {member: offset}) of a struct of include/orbgpu_sim3opt.h, from its text: members in
    order with natural alignment"""
    import re
    text = (ROOT / "include" / "orbgpu_sim3opt.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int": 4, "float": 4, "double": 8}
    off, offsets, align = 0, {}, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for member in rest.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", member)
            sz = sizes[ctype]
            off = (off + sz - 1) // sz * sz
            offsets[m.group(1)] = off
            off += sz * int(m.group(2) or 1)
            align = max(align, sz)
    return (off + align - 1) // align * align, offsets


def test_python_wrapper_and_struct_layout():
    """sizes and offsets agree between ctypes, the numpy dtypes and the header"""
    for cstruct, dtype, name, size in ((sim3opt.Sim3OptJob, sim3opt.JOB_DTYPE, "orbgpu_sim3opt_job", 112),
                                       (sim3opt.Sim3OptResult, sim3opt.RESULT_DTYPE, "orbgpu_sim3opt_result", 160)):
        hsize, hoff = _header_struct(name)
        assert ctypes.sizeof(cstruct) == dtype.itemsize == hsize == size
        assert [f[0] for f in cstruct._fields_] == list(dtype.names) == list(hoff)
        for field in dtype.names:
            assert getattr(cstruct, field).offset == dtype.fields[field][1] == hoff[field], (name, field)
    assert sim3opt.Sim3OptResult.T12.offset == 96 and sim3opt.Sim3OptJob.K1.offset == 72
    z3, z2, z1 = np.zeros((3, 3)), np.zeros((3, 2)), np.zeros(3)
    with pytest.raises(ValueError):
        sim3opt.optimize_sim3_batch(sim3opt.make_jobs([]), z3, z3, z2, np.zeros((2, 2)), z1, z1)
    with pytest.raises(ValueError):
        sim3opt.optimize_sim3_batch(sim3opt.make_jobs([]), z3, z3, z2, z2, z1, z1, removed=np.zeros(3, np.int32))
    e3, e2, e1 = np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0)
    res, out = sim3opt.optimize_sim3_batch(sim3opt.make_jobs([]), e3, e3, e2, e2, e1, e1)
    assert len(res) == 0 and len(out) == 0
    n_in, S, T, out = sim3opt.optimize_sim3((0, 0, 0, 1), (1, 2, 3), 2.0, e3, e3, e2, e2, e1, e1,
                                            (500, 500, 320, 240), (500, 500, 320, 240), 10.0, False)
    assert n_in == 0 and len(out) == 0 and S[2] == 2.0 and list(S[1]) == [1, 2, 3]
    assert T.tolist() == [[2, 0, 0, 1], [0, 2, 0, 2], [0, 0, 2, 3], [0, 0, 0, 1]]


# ---------------------------------------------------------------- the C++ adapter

@pytest.fixture(scope="module")
def sim3opt_main(tmp_path_factory):
    """tests/cpp/sim3opt_main.cpp against Sim3Optimizer.h and the cvlite stand-ins, one g++ line"""
    pkg = ROOT / "orb-slam2-annotation_amd"
    exe = tmp_path_factory.mktemp("sim3opt") / "sim3opt_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'tests' / 'cpp'}", '-DORBGPU_CV_HEADER="cvlite.hpp"', "-pthread", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "sim3opt_main.cpp"), f"-L{pkg}", "-lorbgpu", f"-Wl,-rpath,{pkg}"],
                   check=True)
    return exe


def _adapter_world(s, n_extra, rng):
    """Stand-in keyframes around a scene.  The keyframes get random poses and the MapPoints world
    positions; the correspondences the adapter must gather are then R P + t of those in float (the
    product accumulated in double and rounded once, a float sum: tests/cpp/cvlite_matops.hpp).
    Returns (blob for sim3opt_main, index of the correspondences in vpMatches1, the scene as the
    adapter sees it)."""
    n = len(s["P1c"])
    N1 = n + n_extra
    slots = np.sort(rng.choice(N1, n, replace=False))
    T = []
    for _ in range(2):
        R = synth._rot(rng, 0.4)
        T.append(np.hstack([R, rng.uniform(-1, 1, (3, 1))]).astype(F32))

    def to_world(Pc, Tcw):
        R, t = Tcw[:, :3].astype(np.float64), Tcw[:, 3].astype(np.float64)
        return ((Pc.astype(np.float64) - t) @ R).astype(F32)

    def to_cam(Pw, Tcw):
        R, Pw = Tcw[:, :3].astype(np.float64), Pw.astype(np.float64)
        prod = ((R[:, 0] * Pw[:, 0:1] + R[:, 1] * Pw[:, 1:2]) + R[:, 2] * Pw[:, 2:3]).astype(F32)
        return prod + Tcw[:, 3]

    table = (1.0 / 1.2 ** (2.0 * np.arange(8))).astype(F32)

    def octave(w):
        o = np.rint(np.log(1.0 / w.astype(np.float64)) / (2 * np.log(1.2))).astype(int)
        assert np.array_equal(table[o], w)
        return o
    # MapPoints: 2 per correspondence (keyframe 1's, the match), then the decoys
    Pw1, Pw2 = to_world(s["P1c"], T[0]), to_world(s["P2c"], T[1])
    points = []  # (X, Y, Z, bad, index in keyframe 2)
    rows1 = np.zeros((N1, 5))
    rows1[:, 0:2], rows1[:, 3:5] = (50.0, 60.0), -1
    N2 = n + 5
    order2 = rng.permutation(N2)[:n]  # keyframe 2's keypoint of each correspondence
    rows2 = np.zeros((N2, 3))
    rows2[:, 0:2] = (70.0, 80.0)
    for k, i in enumerate(slots):
        points.append((*Pw1[k], 0, -1))
        points.append((*Pw2[k], 0, order2[k]))
        rows1[i] = (*s["obs1"][k], octave(s["inv_sigma2_1"])[k], 2 * k, 2 * k + 1)
        rows2[order2[k]] = (*s["obs2"][k], octave(s["inv_sigma2_2"])[k])
    # the slots in between: no match; no MapPoint in keyframe 1; a bad MapPoint on either side; a
    # match keyframe 2 does not see -- none is a correspondence, none is touched
    kinds = []
    for i in sorted(set(range(N1)) - set(slots)):
        kind = len(kinds) % 5
        kinds.append(kind)
        base = len(points)
        points.append((1e3, 1e3, 1e3, 1 if kind == 2 else 0, -1))
        points.append((-1e3, 1e3, 1e3, 1 if kind == 3 else 0, -1 if kind == 4 else 0))
        rows1[i, 3] = -1 if kind == 1 else base
        rows1[i, 4] = -1 if kind == 0 else base + 1
    head = [N1, N2, len(points), s["th2"], float(s["fix_scale"]), *s["q12"], *s["t12"], s["s12"],
            *np.array(s["K1"], F32), *np.array(s["K2"], F32), *T[0].reshape(-1), *T[1].reshape(-1), *table]
    blob = np.concatenate([np.array(head, np.float64), rows1.reshape(-1), rows2.reshape(-1),
                           np.array(points, np.float64).reshape(-1)])
    seen = dict(s)
    seen["P1c"], seen["P2c"] = to_cam(Pw1, T[0]), to_cam(Pw2, T[1])
    return blob, slots, rows1[:, 4] >= 0, seen


def _run_adapter(exe, tmp_path, blob):
    (tmp_path / "scene.bin").write_bytes(np.asarray(blob, np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path / "scene.bin"), str(tmp_path / "out.txt")], check=True, timeout=120)
    lines = (tmp_path / "out.txt").read_text().split("\n")
    S = np.array([int(v, 16) for v in lines[1].split()], np.uint64).view(np.float64)
    return int(lines[0]), S, np.array([c == "1" for c in lines[2].strip()], bool)


def test_adapter_builds_and_handles_no_valid_correspondence(sim3opt_main, tmp_path):
    """Sim3Optimizer.h compiles against the stand-ins with -Wall -Wextra; with no valid
    correspondence it needs no GPU: returns 0 and touches neither vpMatches1 nor g2oS12"""
    s = synth.sim3opt_scene(0, 1)
    blob, slots, matched, _ = _adapter_world(s, 10, np.random.default_rng(2))
    assert matched.sum() == 8 and len(slots) == 0
    ret, S, kept = _run_adapter(sim3opt_main, tmp_path, blob)
    assert ret == 0 and np.array_equal(kept, matched) and S.tobytes() == input_bytes(s)


# ---------------------------------------------------------------- GPU

def _torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.gpu
def test_gpu_sizes_in_one_batch():
    _torch_gpu()
    kws = [size_scene(n) for n in SIZES]
    refs = [ref(**kw) for kw in kws]
    scenes = [scene(**kw) for kw in kws]
    jobs, arrays = pack(scenes)
    res, out = sim3opt.optimize_sim3_batch(jobs, *arrays, np.full(len(arrays[0]), 0xA5, np.uint8))
    worst = 0.0
    for k, (j, kw, r, s) in enumerate(zip(jobs, kws, refs, scenes)):
        sl = slice(j["offset"], j["offset"] + j["n"])
        worst = max(worst, check_against_ref(res[k], out[sl], r, s, f"n={kw['n']}"))
    assert [int(v) for v in res["rounds"][:3]] == [0, 1, 1]  # n = 0, 1, 9: S bit-equal (checked above)
    print(f"largest T12 deviation of the size sweep: {worst:.3f} ulp")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases(name):
    """fix_scale on / off, no outliers, a far start with a rejected-then-accepted trial, survivors
    below 10, one point behind keyframe 1"""
    _torch_gpu()
    s, r = scene(**CASES[name]), ref(**CASES[name])
    n_in, S, T, removed = sim3opt.optimize_sim3(s["q12"], s["t12"], s["s12"], *(s[k] for k in KEYS), s["K1"], s["K2"],
                                                s["th2"], s["fix_scale"])
    jobs, arrays = pack([s])
    res, flags = sim3opt.optimize_sim3_batch(jobs, *arrays)
    check_against_ref(res[0], flags, r, s, name)
    assert T.tobytes() == res["T12"][0].tobytes() and np.array_equal(removed, flags.astype(bool)) and n_in == r.n_in
    assert S[2] == res["s12"][0]


def _mixed_scenes(count, seed0):
    sizes = [5, 12, 40, 64, 65, 130, 256, 300, 520, CAP + 40]
    return [synth.sim3opt_scene(sizes[k % len(sizes)], seed0 + k, fix_scale=k % 3 == 1,
                                **(dict(start_rot=0.3, start_t=0.5) if k % 7 == 3 else {})) for k in range(count)]


@pytest.mark.gpu
def test_gpu_batch_invariance_and_determinism():
    """64 jobs of mixed sizes: each job alone gives the bytes it gives in the batch, at any
    position; a second batch call gives the same bytes"""
    _torch_gpu()
    scenes = _mixed_scenes(64, 700)
    jobs, arrays = pack(scenes)
    res, out = sim3opt.optimize_sim3_batch(jobs, *arrays)
    res2, out2 = sim3opt.optimize_sim3_batch(jobs, *arrays)
    assert res.tobytes() == res2.tobytes() and out.tobytes() == out2.tobytes()
    assert (res["rounds"] == np.where(jobs["n"] - res["n_bad_first"] < 10, 1, 2)).all()
    big = jobs["n"] >= 40
    assert (res["n_in"][big] > 0.5 * jobs["n"][big]).all() and (res["n_in"][big] < jobs["n"][big]).all()
    for k, s in enumerate(scenes):
        j1, a1 = pack([s])
        r1, f1 = sim3opt.optimize_sim3_batch(j1, *a1)
        sl = slice(jobs["offset"][k], jobs["offset"][k] + jobs["n"][k])
        assert r1[0].tobytes() == res[k].tobytes() and f1.tobytes() == out[sl].tobytes(), k
    order = np.random.default_rng(1).permutation(64)
    jp, ap = pack([scenes[k] for k in order])
    rp, fp = sim3opt.optimize_sim3_batch(jp, *ap)
    for pos, k in enumerate(order):
        assert rp[pos].tobytes() == res[k].tobytes(), (pos, k)
        assert (fp[jp["offset"][pos]:jp["offset"][pos] + jp["n"][pos]].tobytes() ==
                out[jobs["offset"][k]:jobs["offset"][k] + jobs["n"][k]].tobytes()), (pos, k)


@pytest.mark.gpu
def test_gpu_nan_job_is_isolated_and_the_call_returns():
    """a job whose q12 holds a NaN between two normal jobs, with a gap of unowned correspondences
    before, between and after the jobs: the neighbours' bytes equal those of a batch without it,
    unowned flag bytes and the guard bytes around the device arrays keep their values"""
    torch = _torch_gpu()
    scenes = [synth.sim3opt_scene(n, seed) for n, seed in ((300, 801), (200, 802), (257, 803))]
    gap = 7
    cands, off, cols = [], gap, [[] for _ in KEYS]
    for s in scenes:
        cands.append(job_tuple(s, off))
        off += len(s["P1c"]) + gap
        for col, (k, w) in zip(cols, sim3opt.ARRAYS):
            col += [np.zeros((gap, w), F32), s[k].reshape(-1, w)]
    total = off
    arrays = [np.concatenate(col + [np.zeros((gap, w), F32)]) for col, (_, w) in zip(cols, sim3opt.ARRAYS)]
    arrays[4], arrays[5] = arrays[4].reshape(-1), arrays[5].reshape(-1)
    assert len(arrays[0]) == total
    jobs = sim3opt.make_jobs(cands)
    clean, clean_out = sim3opt.optimize_sim3_batch(jobs[[0, 2]], *arrays, np.full(total, 0xA5, np.uint8))
    jobs["q12"][1][2] = np.nan
    G, RS = 64, sim3opt.RESULT_DTYPE.itemsize
    d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(3, -1)).cuda()
    d_arrays = [torch.from_numpy(a).cuda() for a in arrays]
    res = torch.full((G + 3 * RS + G,), 0xC3, dtype=torch.uint8, device="cuda")
    out = torch.full((G + total + G,), 0xA5, dtype=torch.uint8, device="cuda")
    sim3opt.optimize_sim3_batch_device(d_jobs, *d_arrays, res[G:G + 3 * RS].view(3, RS), out[G:G + total])
    torch.cuda.synchronize()
    res_h, out_h = res.cpu().numpy(), out.cpu().numpy()
    assert (res_h[:G] == 0xC3).all() and (res_h[-G:] == 0xC3).all()
    assert (out_h[:G] == 0xA5).all() and (out_h[-G:] == 0xA5).all()
    got = res_h[G:G + 3 * RS].view(sim3opt.RESULT_DTYPE)
    flags = out_h[G:G + total]
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[1].tobytes()
    owned = np.zeros(total, bool)
    for k in (0, 2):
        sl = slice(jobs["offset"][k], jobs["offset"][k] + jobs["n"][k])
        owned[sl] = True
        assert flags[sl].tobytes() == clean_out[sl].tobytes()
        assert set(np.unique(flags[sl])) <= {0, 1}
    nan_sl = slice(jobs["offset"][1], jobs["offset"][1] + jobs["n"][1])
    owned[nan_sl] = True
    assert (flags[~owned] == 0xA5).all()
    owned[nan_sl] = False
    assert (clean_out[~owned] == 0xA5).all()
    # every chi2 of the NaN job is NaN: the comparisons as written flag nothing, both optimisations run
    assert not flags[nan_sl].any() and got[1]["rounds"] == 2 and got[1]["n_in"] == 200 and got[1]["n_bad_first"] == 0
    assert (got[1]["lm_iterations"] >= 1).all() and (got[1]["lm_iterations"] <= 5).all()


@pytest.mark.gpu
def test_gpu_device_form_on_a_stream():
    """torch tensors on a non-default stream, read after stream.synchronize(); a job with an
    out-of-range offset (which the device form cannot check on the host) gets n_in = rounds = -1"""
    torch = _torch_gpu()
    kws = [size_scene(257), CASES["fix_on"], size_scene(9)]
    scenes, refs = [scene(**kw) for kw in kws], [ref(**kw) for kw in kws]
    jobs, arrays = pack(scenes)
    total = len(arrays[0])
    bad = jobs[:1].copy()
    bad["offset"] = total - 5
    jobs = np.concatenate([jobs, bad])
    RS = sim3opt.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(len(jobs), -1)).cuda()
        d_arrays = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
        d_res = torch.zeros((len(jobs), RS), dtype=torch.uint8, device="cuda")
        d_out = torch.full((total,), 9, dtype=torch.uint8, device="cuda")
    sim3opt.optimize_sim3_batch_device(d_jobs, *d_arrays, d_res, d_out, stream=st)
    st.synchronize()
    res = d_res.cpu().numpy().reshape(-1).view(sim3opt.RESULT_DTYPE)
    out = d_out.cpu().numpy()
    for k, (r, s) in enumerate(zip(refs, scenes)):
        check_against_ref(res[k], out[jobs["offset"][k]:jobs["offset"][k] + jobs["n"][k]], r, s, f"job {k}")
    assert res[3]["rounds"] == -1 and res[3]["n_in"] == -1


@pytest.mark.gpu
def test_gpu_device_form_on_a_second_device():
    torch = _torch_gpu()
    n = orbgpu.device_count()
    if n < 2:
        pytest.skip(f"{n} visible device(s): the second-device call needs >= 2")
    kw = size_scene(257)
    jobs, arrays = pack([scene(**kw)])
    prev = orbgpu.get_thread_device()
    try:
        orbgpu.set_thread_device(1)
        with torch.cuda.device(1):
            dev = torch.device("cuda", 1)
            t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (jobs.view(np.uint8).reshape(1, -1), *arrays)]
            d_res = torch.zeros((1, sim3opt.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            d_out = torch.zeros(len(arrays[0]), dtype=torch.uint8, device=dev)
            sim3opt.optimize_sim3_batch_device(*t, d_res, d_out, stream=torch.cuda.current_stream(dev))
            torch.cuda.synchronize(dev)
            res = d_res.cpu().numpy().reshape(-1).view(sim3opt.RESULT_DTYPE)
            check_against_ref(res[0], d_out.cpu().numpy(), ref(**kw), scene(**kw), "device 1")
    finally:
        orbgpu.set_thread_device(prev)


@pytest.mark.gpu
def test_gpu_adapter(sim3opt_main, tmp_path):
    """OptimizeSim3GPU on stand-in keyframes with unmatched, null, bad and unseen MapPoints
    interleaved: vpMatches1 is NULL exactly where the restatement removes a correspondence (and
    where it was NULL before), g2oS12 and the return value equal the restatement's on the
    correspondences as the adapter's float product forms them; a scene that ends with fewer than
    10 survivors returns 0, keeps the first check's flags and leaves g2oS12 alone"""
    _torch_gpu()
    for kw, extra in ((size_scene(255), 145), (CASES["few"], 6)):
        blob, slots, matched, seen = _adapter_world(scene(**kw), extra, np.random.default_rng(3))
        r = run_ref(seen)
        assert sim3opt_ref.threshold_margin(r, seen["th2"]) >= MARGIN
        ret, S, kept = _run_adapter(sim3opt_main, tmp_path, blob)
        expect = matched.copy()
        expect[slots[r.removed]] = False
        assert ret == r.n_in and np.array_equal(kept, expect)
        if r.rounds < 2:
            assert S.tobytes() == input_bytes(seen) and ret == 0 and r.removed.any()
        else:
            got = (list(S[:4]), list(S[4:7]), float(S[7]))
            dev = t12_deviation(sim3opt_ref.sim3_to_T(got), r.T12)
            print(f"adapter: T12 deviation {dev:.3f} ulp")
            assert dev <= ULP_BOUND and S.tobytes() != input_bytes(seen)
