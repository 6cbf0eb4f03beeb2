"""Local bundle adjustment (include/orbgpu_localba.h, csrc/localba.hip,
include/orbslam2_amd/LocalBundleAdjuster.h) against the numpy restatement of
Optimizer::LocalBundleAdjustment (tests/localba_ref.py).

Parity: every element of every local pose within ULP_BOUND float32 ulps at the
scale max(1, max|.|) of that pose, every point coordinate within the same bound
at the scale max(1, max|.|) of the job's points; erase flags, n_bad_first,
n_erase and rounds equal; LM counters in range only.  The kernel and the
restatement sum a vertex's block in the same order, but associate the robust
chi2 and computeScale's sum differently, and accept / reject at convergence is
decided by such rounding.  The bound is therefore measured, not fixed (the rule
and reasons of test_sim3opt.py): MEASURED_WORST is the largest deviation the
restatement shows on any regular fixture when its points are permuted and its
edges are permuted within each point (8 permutations each), and ULP_BOUND =
max(2, 4 x MEASURED_WORST).  test_ref_permutation_spread_of_every_fixture asserts
the measurement.  The degenerate fixtures -- points left with a single
monocular edge, whose depth only the damping holds ("single", and "depth_only",
whose single-edge point starts behind its camera), and a job with no fixed pose
at all, whose gauge only the damping holds ("nofixed") -- have their own
measured bounds by the same rule (DEGENERATE below).

Every scene's seed is fixed and chosen on the CPU so that, in the restatement
and under each of the 8 permutations, every chi2 either check reads is at least
1e-6 (relative) from its threshold and every depth either check reads is at
least 1e-6 from 0; the tests assert that before they compare.

Measured on the CPU, the restatement under permutation: 0.000 ulp on every
fixture, the degenerate ones included, so every bound is the floor, 2 ulp.
Measured on an MI355X against the restatement: 0.000 ulp on all 15 fixtures of
the size sweep, on all 7 named cases, on the device form and through the C++
adapter (every float32 pose element and point coordinate equal), with the erase
flags, n_bad_first, n_erase, rounds and, as it happened, the LM counters equal
everywhere.
"""
import ctypes
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import localba
import localba_ref
import orbgpu
import poseopt_ref
import synth

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
ULP = 2.0 ** -23
MARGIN = 1e-6
PERMUTATIONS = 8
THREADS = 256  # csrc/localba.hip: the workgroup size, the kernel's only capacity constant
# the restatement's worst deviation under 8 permutations of any regular fixture, measured on the CPU:
# 0.000 ulp on every fixture (the doubles differ near 1e-13 relative, which did not cross a float32
# rounding boundary anywhere), so the bound is the floor
MEASURED_WORST = 0.0
ULP_BOUND = max(2.0, 4.0 * MEASURED_WORST)
# the degenerate fixtures: their own measured worst, and the bound made from it by the same rule
# (all three measured 0.000 ulp: their bound is the floor, 2)
DEGENERATE = {"single": 0.0, "nofixed": 0.0, "depth_only": 0.0}


def bound_of(label):
    return max(2.0, 4.0 * DEGENERATE[label]) if label in DEGENERATE else ULP_BOUND


ALL = dict(see=1.0)  # every camera sees every point: the edge count is poses x points
# the size sweep: free poses 1, 2, 3, 6; fixed poses 0 (kf0_local), 1, 3; points 1, 2, 15, 16, 17, 63,
# 64, 65, 300; 63 / 64 / 65 edges around the wave, 255 / 256 / 260 around THREADS; mono only, stereo
# only, mixed; no edge at all; every pose fixed.  p17_kf0's seed (searched from 217 upwards) makes the
# quaternion round trip of its fixed local pose change two of the pose's float32 elements
SIZES = {
    "p1": dict(n_local=1, n_fixed=1, n_points=1, seed=201),
    "p2": dict(n_local=2, n_fixed=1, n_points=2, seed=202, **ALL),
    "p15": dict(n_local=3, n_fixed=1, n_points=15, seed=215, stereo=1.0),
    "p16_e64": dict(n_local=2, n_fixed=2, n_points=16, seed=216, **ALL),
    "p17_kf0": dict(n_local=3, n_fixed=0, n_points=17, seed=243, stereo=1.0, kf0_local=True),
    "e63": dict(n_local=2, n_fixed=1, n_points=21, seed=221, stereo=0.5, **ALL),
    "e65": dict(n_local=2, n_fixed=3, n_points=13, seed=213, **ALL),
    "p63": dict(n_local=2, n_fixed=1, n_points=63, seed=263, stereo=0.3),
    "p64_e256": dict(n_local=1, n_fixed=3, n_points=64, seed=264, **ALL),
    "e255": dict(n_local=3, n_fixed=2, n_points=51, seed=251, stereo=0.5, **ALL),
    "e260": dict(n_local=3, n_fixed=2, n_points=52, seed=252, **ALL),
    "p65": dict(n_local=6, n_fixed=1, n_points=65, seed=265, stereo=0.5, outliers=0.05),
    "p300": dict(n_local=6, n_fixed=3, n_points=300, seed=300, stereo=0.3, outliers=0.05),
    "e0": dict(n_local=2, n_fixed=1, n_points=0, seed=200),
    "all_fixed": dict(n_local=2, n_fixed=2, n_points=16, seed=230, fix_all=True, **ALL),
}
# `far`: a start 0.15 rad / 0.5 m off (points 0.5 m) whose trace in the restatement has a rejected
# trial followed by an accepted one; `spoil_point` / `spoil_pose`: every observation of that point /
# by that local pose is moved 40 px, so all its edges are flagged after the first round;
# `depth_only`: point 0 has one monocular observation and starts mirrored through that camera;
# `single`: three points with one monocular observation each; `nofixed`: no fixed pose at all
CASES = {
    "far": dict(n_local=3, n_fixed=2, n_points=40, seed=1, stereo=0.5, noise=0.5, start_rot=0.15, start_t=0.5,
                start_pt=0.5),
    "clean": dict(n_local=4, n_fixed=2, n_points=60, seed=31, noise=0.5, stereo=0.3),
    "all_flagged_point": dict(n_local=3, n_fixed=2, n_points=30, seed=41, stereo=0.3, spoil_point=7, **ALL),
    "all_flagged_pose": dict(n_local=3, n_fixed=2, n_points=30, seed=51, stereo=0.3, spoil_pose=1, **ALL),
    "depth_only": dict(n_local=3, n_fixed=2, n_points=30, seed=61, single_obs=1, behind=True),
    "single": dict(n_local=3, n_fixed=2, n_points=30, seed=71, single_obs=3),
    "nofixed": dict(n_local=3, n_fixed=0, n_points=40, seed=81, stereo=1.0, **ALL),
}


@functools.lru_cache(maxsize=None)
def _scene_cached(items):
    kw = dict(items)
    fix_all, spoil_point, spoil_pose = kw.pop("fix_all", False), kw.pop("spoil_point", None), kw.pop("spoil_pose", None)
    s = synth.localba_scene(**kw)
    if fix_all:
        s["fixed"][:] = 1
    for key, idx in (("point_idx", spoil_point), ("pose_idx", spoil_pose)):
        if idx is not None:
            sel = np.nonzero(s[key] == idx)[0]
            ang = 0.7 + 2.4 * np.arange(len(sel))
            s["obs"][sel, 0] += F32(40.0) * np.cos(ang).astype(F32)
            s["obs"][sel, 1] += F32(40.0) * np.sin(ang).astype(F32)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def scene(**kw):
    return _scene_cached(tuple(sorted(kw.items())))


def check_margins(r, s, what):
    m_chi, m_z = localba_ref.margins(r, s["obs"])
    assert m_chi >= MARGIN and m_z >= MARGIN, (what, m_chi, m_z)


@functools.lru_cache(maxsize=None)
def _ref_cached(items):
    return localba_ref.run_scene(_scene_cached(items))


def ref(**kw):
    """the restatement's result of a scene, computed once per session, with the margin precondition"""
    r = _ref_cached(tuple(sorted(kw.items())))
    check_margins(r, scene(**kw), kw)
    return r


def all_fixtures():
    return list(SIZES.items()) + list(CASES.items())


def deviation(T, X, r):
    """largest deviation of the float32 local poses T (n, 4, 4) and points X (M, 3) from the
    restatement's in float32 ulps, a pose at its own scale, the points at the job's"""
    dev = 0.0
    for a, b in zip(T.reshape(-1, 4, 4), r.Tcw):
        scale = max(1.0, float(np.abs(b).max()))
        dev = max(dev, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / (ULP * scale))
    if len(r.Xw):
        scale = max(1.0, float(np.abs(r.Xw).max()))
        dev = max(dev, float(np.abs(X.astype(np.float64) - r.Xw.astype(np.float64)).max()) / (ULP * scale))
    return dev


def job_slices(j):
    return (slice(j["out_pose_offset"], j["out_pose_offset"] + j["n_local"]),
            slice(j["point_offset"], j["point_offset"] + j["n_points"]),
            slice(j["edge_offset"], j["edge_offset"] + j["n_edges"]))


def check_against_ref(res, T, X, erase, r, label):
    """one job's record, local poses, points and erase bytes against the restatement; returns the
    deviation in ulps.  Every pose, point and edge of the job is compared."""
    bound = bound_of(label)
    assert T.shape == (len(r.Tcw), 16) and X.shape == r.Xw.shape and erase.shape == r.erase.shape, label
    dev = deviation(T, X, r)
    print(f"{label}: deviation {dev:.3f} ulp (bound {bound:.3f}), rounds {res['rounds']}, n_bad_first "
          f"{res['n_bad_first']}, n_erase {res['n_erase']}, iterations {list(res['lm_iterations'])}, rejected "
          f"{list(res['lm_rejected'])}; restatement {[(t.iterations, t.rejected) for t in r.trace]}")
    assert set(np.unique(erase)) <= {0, 1}, label
    assert np.array_equal(erase.astype(bool), r.erase), (label, int((erase.astype(bool) != r.erase).sum()))
    assert (int(res["rounds"]), int(res["n_bad_first"]), int(res["n_erase"])) == (r.rounds, r.n_bad_first, r.n_erase), label
    assert dev <= bound, (label, dev)
    assert np.array_equal(T[:, 12:], np.tile(F32([0, 0, 0, 1]), (len(T), 1))), label
    for k, limit in enumerate(localba_ref.ITERATIONS):
        if r.rounds:
            assert 0 <= res["lm_iterations"][k] <= limit and 0 <= res["lm_rejected"][k] <= 10 * limit, label
        else:
            assert res["lm_iterations"][k] == 0 and res["lm_rejected"][k] == 0, label
    return dev


def run_batch(scenes):
    jobs, a = localba.make_batch(scenes)
    return (jobs, *localba.local_ba_batch(jobs, *(a[n] for n, *_ in localba.INPUTS)))


def permuted(s, k):
    M = len(s["Xw"])
    return localba_ref.run_scene(s, np.random.default_rng(1000 + k).permutation(M), 2000 + k)


# ---------------------------------------------------------------- CPU: the restatement's own checks

def test_ref_jacobians_agree_with_central_differences():
    """both analytic Jacobians of both edges against central differences of the restatement's own
    error function (the stereo invz kept in double there: the float rounding is not smooth)"""
    s = scene(**SIZES["e63"])
    job = localba_ref.make_job(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"], s["obs"],
                               s["inv_sigma2"], s["n_local"])
    assert job.stereo.any() and (~job.stereo).any()
    Q = np.array([poseopt_ref.se3_from_T(T)[0] for T in job.Tcw])
    Tt = np.array([poseopt_ref.se3_from_T(T)[1] for T in job.Tcw])
    pts = job.Xw.astype(np.float64)
    _, _, p = localba_ref.edge_errors(Q, Tt, pts, job, float_invz=False)
    Jl, Jp = localba_ref.edge_jacobians(Q, p, job)
    h = 1e-6

    def err(Q_, Tt_, pts_):
        return localba_ref.edge_errors(Q_, Tt_, pts_, job, float_invz=False)[0]

    worst = 0.0
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        num = (err(Q, Tt, pts + d) - err(Q, Tt, pts - d)) / (2 * h)
        worst = max(worst, float(np.abs(num - Jl[:, :, c]).max() / np.abs(Jl).max()))
    for c in range(6):
        sides = []
        for sign in (1.0, -1.0):
            x = [0.0] * 6
            x[c] = sign * h
            Q2, T2 = Q.copy(), Tt.copy()
            for k in range(job.P):
                Q2[k], T2[k] = poseopt_ref.se3_mul(poseopt_ref.se3_exp(x), (list(Q[k]), list(Tt[k])))
            sides.append(err(Q2, T2, pts))
        num = (sides[0] - sides[1]) / (2 * h)
        worst = max(worst, float(np.abs(num - Jp[:, :, c]).max() / np.abs(Jp).max()))
    print(f"largest relative difference of analytic and numeric Jacobians: {worst:.2e}")
    # truncation h^2 |f'''| / 6 and rounding eps |f| / h of a central difference with h = 1e-6 on
    # errors of hundreds of pixels: both below 1e-7 of the largest Jacobian entry
    assert worst < 1e-7


@pytest.mark.parametrize("name", ["p15", "e63", "p17_kf0"])
def test_ref_schur_solve_agrees_with_the_dense_solve(name):
    """x of the Schur complement, the reduced Cholesky and the back-substitution against
    numpy.linalg.solve on the whole damped system assembled densely"""
    s = scene(**SIZES[name])
    job = localba_ref.make_job(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"], s["point_idx"], s["obs"],
                               s["inv_sigma2"], s["n_local"])
    st = localba_ref.structure(job, np.zeros(job.E, bool))
    Q = np.array([poseopt_ref.se3_from_T(T)[0] for T in job.Tcw])
    Tt = np.array([poseopt_ref.se3_from_T(T)[1] for T in job.Tcw])
    system = localba_ref.build_system((Q, Tt, job.Xw.astype(np.float64)), job, st, True, np.zeros(job.E))
    nf, M = st.nf, job.M
    assert nf >= 2 and st.nl == M
    N = 6 * nf + 3 * M
    free = np.nonzero(st.pose_free)[0]
    for lam in (1e-5 * max(np.abs(system.Hpp).max(), np.abs(system.Hll).max()), 10.0):
        H, b = np.zeros((N, N)), np.zeros(N)
        for i, p in enumerate(free):
            H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = system.Hpp[p]
            b[6 * i:6 * i + 6] = system.bp[p]
        for m in range(M):
            o = 6 * nf + 3 * m
            H[o:o + 3, o:o + 3] = system.Hll[m]
            b[o:o + 3] = system.bl[m]
        for e in st.ef:
            i, o = st.hidx[job.pose_idx[e]], 6 * nf + 3 * job.point_idx[e]
            H[6 * i:6 * i + 6, o:o + 3] += system.B[e]
            H[o:o + 3, 6 * i:6 * i + 6] += system.B[e].T
        H += lam * np.eye(N)
        xp, xl = localba_ref.schur_solve(system, job, st, lam)
        x = np.concatenate([xp.reshape(-1), xl.reshape(-1)])
        x_dense = np.linalg.solve(H, b)
        cond = np.linalg.cond(H)
        rel = float(np.linalg.norm(x - x_dense) / np.linalg.norm(x_dense))
        # two backward-stable solves of a symmetric positive definite system of N unknowns: each is
        # within N eps cond(H) of the exact solution in the 2-norm
        bound = 2 * N * np.finfo(np.float64).eps * cond
        print(f"{name}, lambda {lam:.3g}: N {N}, cond {cond:.3g}, relative difference {rel:.3g}, bound {bound:.3g}")
        assert rel <= bound


def test_ref_noise_free_flags_exactly_the_injected_outliers():
    """noise-free observations, every point seen by all 7 cameras, 5 % of the observations 30-80 px
    off: exactly those are erased, and the poses and points come back to the truth.  The noise floor
    is the float32 rounding of the observations (half an ulp at 512-1024 px: 3e-5 px, 6e-8 rad at
    f = 517), which over the narrowest triangulation angle of the arc (0.08 rad) at 12 m is 1e-5 m
    in a point and less in a pose; the bounds are ten times that, 1e-4 m and 1e-5."""
    kw = dict(n_local=4, n_fixed=3, n_points=60, seed=91, noise=0.0, outliers=0.05, stereo=0.3, **ALL)
    s, r = scene(**kw), ref(**kw)
    assert 0 < s["outlier"].sum() < 0.1 * len(s["outlier"])
    assert np.array_equal(r.erase, s["outlier"]) and np.array_equal(r.flag_first, s["outlier"])
    assert r.n_erase == r.n_bad_first == int(s["outlier"].sum()) and r.rounds == 2
    pose_err = float(np.abs(r.Tcw.astype(np.float64) - s["Tcw_true"][:4]).max())
    point_err = float(np.abs(r.Xw.astype(np.float64) - s["Xw_true"]).max())
    start = float(np.abs(s["Tcw"][:4].astype(np.float64) - s["Tcw_true"][:4]).max())
    print(f"pose error {pose_err:.2e} (start {start:.2e}), point error {point_err:.2e}")
    assert start > 1e-2 and pose_err < 1e-5 and point_err < 1e-4


def test_ref_a_point_without_an_active_edge_keeps_its_first_round_estimate():
    kw = CASES["all_flagged_point"]
    s, r = scene(**kw), ref(**kw)
    m = kw["spoil_point"]
    mine = s["point_idx"] == m
    assert mine.sum() == 5 and r.flag_first[mine].all() and not r.flag_first[~mine].all()
    assert r.est[2][m].tobytes() == r.est_first[2][m].tobytes()
    moved = [k for k in range(len(s["Xw"])) if r.est[2][k].tobytes() != r.est_first[2][k].tobytes()]
    assert len(moved) == len(s["Xw"]) - 1  # every other point was optimised again
    assert r.Xw[m].tobytes() == r.est_first[2][m].astype(F32).tobytes()


def test_ref_a_local_pose_without_an_active_edge_keeps_its_first_round_estimate():
    kw = CASES["all_flagged_pose"]
    s, r = scene(**kw), ref(**kw)
    p = kw["spoil_pose"]
    mine = s["pose_idx"] == p
    assert mine.sum() == 30 and r.flag_first[mine].all() and not s["fixed"][p]
    for a in (0, 1):
        assert r.est[a][p].tobytes() == r.est_first[a][p].tobytes()
        for other in (0, 2):
            assert r.est[a][other].tobytes() != r.est_first[a][other].tobytes()
    assert r.Tcw[p].tobytes() == poseopt_ref.se3_to_T((list(r.est_first[0][p]), list(r.est_first[1][p]))).tobytes()


def test_ref_an_edge_flagged_for_depth_only_keeps_its_stale_chi2():
    """point 0 has one monocular edge and starts mirrored through its camera: chi2 is small, the
    depth negative.  The first test flags the edge for its depth alone; in the second optimisation
    it is at level 1, its chi2() stays the first round's value, and the final test erases it on the
    depth at the final estimates"""
    kw = CASES["depth_only"]
    s, r = scene(**kw), ref(**kw)
    e = int(np.nonzero(s["point_idx"] == 0)[0][0])
    assert (s["point_idx"] == 0).sum() == 1 and s["obs"][e, 2] < 0
    assert r.flag_first[e] and r.chi2_first[e] < 5.991 * (1 - MARGIN) and r.z_first[e] < 0
    assert r.erase[e] and r.chi2_final[e] == r.chi2_first[e] and r.z_final[e] < 0
    assert r.z_final[e] != r.z_first[e]  # the pose moved on: the depth test read the final estimates
    assert r.est[2][0].tobytes() == r.est_first[2][0].tobytes()
    others = np.arange(len(s["obs"])) != e
    assert (r.chi2_final[others & ~r.flag_first] != r.chi2_first[others & ~r.flag_first]).all()


def test_ref_no_edge_means_no_round_and_a_fixed_local_pose_is_round_tripped():
    s, r = scene(**SIZES["e0"]), ref(**SIZES["e0"])
    assert r.rounds == 0 and r.n_erase == 0 and r.trace == [] and len(r.erase) == 0 and r.Tcw.shape == (2, 4, 4)
    # a fixed local pose (keyframe 0) leaves as Converter::toCvMat(toSE3Quat(.)) of its input: not its bits
    kw = SIZES["p17_kf0"]
    s, r = scene(**kw), ref(**kw)
    assert s["fixed"][0] and not s["fixed"][1]
    trip = poseopt_ref.se3_to_T(poseopt_ref.se3_from_T(s["Tcw"][0]))
    assert r.Tcw[0].tobytes() == trip.tobytes() and r.Tcw[0].tobytes() != s["Tcw"][0].tobytes()
    assert np.abs(r.Tcw[0] - s["Tcw"][0]).max() <= 4 * ULP * max(1.0, np.abs(s["Tcw"][0]).max())


@pytest.mark.parametrize("label,kw", all_fixtures(), ids=[label for label, _ in all_fixtures()])
def test_ref_permutation_spread_of_every_fixture(label, kw):
    """the same scene with its points permuted and its edges permuted within each point (every sum
    rounds differently), 8 times: the margins hold, the integer outcomes are equal, and poses and
    points stay within the measured worst the GPU bound is made from"""
    s, a = scene(**kw), ref(**kw)
    worst = 0.0
    for k in range(PERMUTATIONS):
        b = permuted(s, k)
        check_margins(b, s, (label, k))
        assert np.array_equal(a.erase, b.erase) and np.array_equal(a.flag_first, b.flag_first)
        assert (a.rounds, a.n_bad_first, a.n_erase) == (b.rounds, b.n_bad_first, b.n_erase)
        worst = max(worst, deviation(b.Tcw.reshape(-1, 16), b.Xw, a))
    print(f"{label}: permutation spread {worst:.3f} ulp")
    measured = DEGENERATE[label] if label in DEGENERATE else MEASURED_WORST
    assert worst <= measured + 1e-3


def test_scene_preconditions():
    """what the named fixtures are for holds in the restatement"""
    for label, kw in all_fixtures():
        r = ref(**kw)
        assert r.rounds == (0 if label == "e0" else 2), label
    found = False
    for tr in ref(**CASES["far"]).trace:
        for k in range(1, len(tr.trials)):
            if not tr.trials[k - 1] and tr.trials[k]:
                found = True
    assert found
    r = ref(**CASES["clean"])
    assert r.n_bad_first == 0 and r.n_erase == 0
    for name in ("p65", "p300"):
        r = ref(**SIZES[name])
        assert 0 < r.n_bad_first and 0 < r.n_erase < len(r.erase) // 4
    s = scene(**CASES["single"])
    assert sorted(np.bincount(s["point_idx"]))[:3] == [1, 1, 1]
    s = scene(**CASES["nofixed"])
    assert not s["fixed"].any()
    s = scene(**SIZES["all_fixed"])
    r = ref(**SIZES["all_fixed"])
    assert s["fixed"].all() and r.rounds == 2 and all(t.iterations >= 1 for t in r.trace)
    counts = sorted(len(scene(**kw)["obs"]) for kw in SIZES.values())
    for n in (0, 63, 64, 65, THREADS - 1, THREADS, THREADS + 4):
        assert n in counts, n
    assert {kw["n_points"] for kw in SIZES.values()} >= {0, 1, 2, 15, 16, 17, 63, 64, 65, 300}


# ---------------------------------------------------------------- CPU: argument checks of the library

ARRAY_ARGS = tuple(n for n, *_ in localba.INPUTS) + tuple(n for n, *_ in localba.OUTPUTS)


def _jobs2(**kw):
    rows = [dict(n_poses=3, n_local=2, n_points=4, n_edges=6, pose_offset=0, point_offset=0, edge_offset=0, out_pose_offset=0),
            dict(n_poses=2, n_local=1, n_points=3, n_edges=4, pose_offset=3, point_offset=4, edge_offset=6, out_pose_offset=2)]
    for key, val in kw.items():
        rows[int(key[-1])][key[:-1]] = val
    return localba.make_jobs([tuple(r[n] for n in localba.JOB_DTYPE.names) for r in rows])


def _edges2(pose=None, point=None):
    ep = np.array([0, 1, 2, 0, 1, 2, 0, 1, 0, 1], np.int32)
    el = np.array([0, 0, 1, 2, 3, 3, 0, 1, 2, 2], np.int32)
    if pose:
        ep[pose[0]] = pose[1]
    if point:
        el[point[0]] = point[1]
    return ep, el


def _args(form, **kw):
    """the library call with fake non-null pointers (never dereferenced by a rejected call), real
    jobs and edge indices for the host form's per-job checks"""
    a = dict(batch=2, jobs=_jobs2(), tp=5, tl=3, tm=7, te=10, max_local=2, res=1 << 20, ws=1 << 30, ws_bytes=1 << 40)
    a.update({name: 1 << (21 + k) for k, name in enumerate(ARRAY_ARGS)})
    ep, el = _edges2()
    a["edge_pose"], a["edge_point"] = ep, el
    a.update(kw)
    ptr = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    jobs = a["jobs"]
    jp = None if jobs is None else (jobs.ctypes.data if form == "host" else 1 << 22)
    arrays = [ptr(a[name]) if form == "host" or a[name] is None else 1 << 23 for name in ARRAY_ARGS]
    L = orbgpu.lib()
    head = (a["batch"], jp, a["tp"], a["tl"], a["tm"], a["te"], a["max_local"])
    if form == "host":
        return L.orbgpu_local_ba_batch(*head, *arrays, a["res"], a["ws"], a["ws_bytes"])
    return L.orbgpu_local_ba_batch_device(*head, *arrays, a["res"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_checks_need_no_device(form):
    """rejected on the host before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    for name in ("batch", "tp", "tl", "tm", "te", "max_local"):
        assert _args(form, **{name: -1}) == E, name
    for name in ("jobs", *ARRAY_ARGS, "res"):
        assert _args(form, **{name: None}) == E, name
        assert "null" in orbgpu.last_error(), name
    need = localba.workspace_bytes(2, 5, 7, 10, 2)
    assert need > 0 and need % 8 == 0
    assert _args(form, ws_bytes=need - 1) == E and "workspace" in orbgpu.last_error()
    assert _args(form, ws=(1 << 30) + 4) == E
    if form == "device":
        assert _args(form, ws=None) == E
    assert _args(form, batch=0) == orbgpu.OK
    none = {name: None for name in ARRAY_ARGS}
    assert _args(form, batch=0, tp=0, tl=0, tm=0, te=0, jobs=None, res=None, ws=None, ws_bytes=0, **none) == orbgpu.OK
    assert localba.workspace_bytes(-1, 0, 0, 0, 0) == 0
    assert localba.workspace_bytes(3, 5, 7, 10, 2) > need > localba.workspace_bytes(2, 5, 7, 9, 2)


def test_job_range_and_index_checks_need_no_device():
    E = orbgpu.ERR_ARG
    for bad in (dict(n_poses0=-1), dict(n_edges1=-1), dict(pose_offset0=-1), dict(n_poses1=3), dict(n_points1=4),
                dict(n_edges1=5), dict(out_pose_offset1=3), dict(n_local0=4), dict(n_local1=3),
                dict(edge_offset1=2 ** 31 - 1, n_edges1=2 ** 31 - 1)):
        assert _args("host", jobs=_jobs2(**bad)) == E, bad
        assert "job %s" % list(bad)[0][-1] in orbgpu.last_error(), bad
    assert _args("host", max_local=1) == E and "job 0" in orbgpu.last_error()  # n_local 2 > max_local
    for pose in ((2, 3), (2, -1), (8, 2)):  # job 0 has 3 poses, job 1 has 2
        ep, el = _edges2(pose=pose)
        assert _args("host", edge_pose=ep, edge_point=el) == E and "out of range" in orbgpu.last_error(), pose
    for point in ((5, 4), (0, -1), (9, 3)):
        ep, el = _edges2(point=point)
        assert _args("host", edge_pose=ep, edge_point=el) == E and "out of range" in orbgpu.last_error(), point
    ep, el = _edges2(point=(3, 0))  # 0 0 1 0: decreasing
    assert _args("host", edge_pose=ep, edge_point=el) == E and "decrease" in orbgpu.last_error()
    ep, el = _edges2(point=(8, 0))
    assert _args("host", edge_pose=ep, edge_point=el) == E and "job 1" in orbgpu.last_error()


def _header_struct(name):
    """(size, {member: offset}) of a struct of include/orbgpu_localba.h, from its text"""
    text = (ROOT / "include" / "orbgpu_localba.h").read_text()
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
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", member)
            offsets[m.group(1)] = off
            off += 4 * int(m.group(2) or 1)
    return off, offsets


def test_python_wrapper_and_struct_layout():
    """sizes and offsets agree between ctypes, the numpy dtypes and the header"""
    for cstruct, dtype, name in ((localba.LocalBAJob, localba.JOB_DTYPE, "orbgpu_localba_job"),
                                 (localba.LocalBAResult, localba.RESULT_DTYPE, "orbgpu_localba_result")):
        hsize, hoff = _header_struct(name)
        assert ctypes.sizeof(cstruct) == dtype.itemsize == hsize == 32
        assert [f[0] for f in cstruct._fields_] == list(dtype.names) == list(hoff)
        for field in dtype.names:
            assert getattr(cstruct, field).offset == dtype.fields[field][1] == hoff[field], (name, field)
    jobs, a = localba.make_batch([scene(**SIZES["p2"]), scene(**SIZES["e0"]), scene(**SIZES["p15"])])
    assert jobs["pose_offset"].tolist() == [0, 3, 6] and jobs["out_pose_offset"].tolist() == [0, 2, 4]
    assert jobs["n_edges"].tolist()[:2] == [6, 0] and a["Tcw"].shape == (10, 12) and a["edge_pose"].dtype == np.int32
    with pytest.raises(ValueError):
        localba.local_ba_batch(jobs, a["Tcw"], a["fixed"][:-1], *(a[n] for n, *_ in localba.INPUTS[2:]))
    with pytest.raises(ValueError):
        localba.local_ba_batch(jobs, *(a[n] for n, *_ in localba.INPUTS), erase=np.zeros(len(a["obs"]), np.int32))
    res, T, X, er = localba.local_ba_batch(localba.make_jobs([]), *localba.make_batch([])[1].values())
    assert len(res) == 0 and T.shape == (0, 16) and X.shape == (0, 3) and len(er) == 0


# ---------------------------------------------------------------- the C++ adapter

@pytest.fixture(scope="module")
def localba_main(tmp_path_factory):
    """tests/cpp/localba_main.cpp against LocalBundleAdjuster.h and the cvlite stand-ins, one g++ line"""
    pkg = ROOT / "orb-slam2-annotation_amd"
    exe = tmp_path_factory.mktemp("localba") / "localba_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'tests' / 'cpp'}", '-DORBGPU_CV_HEADER="cvlite.hpp"', "-pthread", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "localba_main.cpp"), f"-L{pkg}", "-lorbgpu", f"-Wl,-rpath,{pkg}"],
                   check=True)
    return exe


TABLE = (1.0 / 1.2 ** (2.0 * np.arange(8))).astype(F32)


def _adapter_world(s, rng, with_points=True):
    """Stand-in keyframes and MapPoints around a scene, with what the gather must skip interleaved: a
    bad covisible keyframe, a bad fixed keyframe (both observe points), null and bad MapPoints in the
    keyframes' match lists, and keyframe 0 as a local keyframe.  Keyframe indices are shuffled, so
    GetObservations() (ordered by keyframe index) is not the scene's order.  Returns (blob for
    localba_main, the problem as the gather must produce it, the keyframe index of each of its poses,
    the MapPoint index of each of its points)."""
    P, M, NL = len(s["Tcw"]), len(s["Xw"]), s["n_local"]
    n_kf = P + 2                                  # + a bad neighbour, + a bad outside observer
    kf_of_pose = rng.permutation(n_kf)[:P]        # scene pose -> keyframe index
    spare = sorted(set(range(n_kf)) - set(kf_of_pose.tolist()))
    bad_neighbour, bad_observer = spare
    octave = np.rint(np.log(1.0 / s["inv_sigma2"].astype(np.float64)) / (2 * np.log(1.2))).astype(int)
    assert np.array_equal(TABLE[octave], s["inv_sigma2"])
    n_mp = (M if with_points else 0) + 2          # + a bad MapPoint, + one only the bad keyframes see
    mp_of_point = rng.permutation(n_mp)[:M] if with_points else np.zeros(0, int)
    spare_mp = sorted(set(range(n_mp)) - set(mp_of_point.tolist()))
    bad_mp = spare_mp[0]
    keys = [[] for _ in range(n_kf)]              # per keyframe: (x, y, octave, uRight, MapPoint or -1)
    obs_of = [[] for _ in range(n_mp)]            # per MapPoint: (keyframe, keypoint)
    if with_points:
        for e in range(len(s["obs"])):
            k, m = int(kf_of_pose[s["pose_idx"][e]]), int(mp_of_point[s["point_idx"][e]])
            if len(keys[k]) % 3 == 1:
                keys[k].append((5.0, 6.0, 0, -1.0, -1))           # a null MapPoint in between
            if len(keys[k]) % 7 == 3:
                keys[k].append((7.0, 8.0, 1, -1.0, bad_mp))       # a bad one: not gathered
                obs_of[bad_mp].append((k, len(keys[k]) - 1))
            keys[k].append((*s["obs"][e][:2], octave[e], s["obs"][e][2], m))
            obs_of[m].append((k, len(keys[k]) - 1))
        # the bad keyframes observe the first points: no edge, no vertex
        for k in (bad_neighbour, bad_observer):
            for m in mp_of_point[:3]:
                keys[k].append((11.0, 12.0, 0, -1.0, int(m)))
                obs_of[int(m)].append((k, len(keys[k]) - 1))
    # the current keyframe is the first local pose, unless that is keyframe 0 (whose id the marks of
    # every MapPoint start with): then the second
    local_order = list(range(NL))
    if NL > 1 and s["fixed"][0]:
        local_order[0], local_order[1] = 1, 0
    cur = int(kf_of_pose[local_order[0]])
    # covisible keyframes of the current one: the other local ones in that order, the bad one second
    cov = [int(kf_of_pose[p]) for p in local_order[1:]]
    cov.insert(min(1, len(cov)), bad_neighbour)
    # mnId: keyframe 0 is the fixed local pose when the scene has one; ids otherwise distinct and >= 1
    ids = np.arange(1, n_kf + 1) * 3
    fixed_local = [p for p in range(NL) if s["fixed"][p]]
    assert len(fixed_local) <= 1
    for p in fixed_local:
        ids[kf_of_pose[p]] = 0
    blob = [n_kf, n_mp, cur, 0.0, *TABLE]
    for k in range(n_kf):
        pose = np.nonzero(kf_of_pose == k)[0]
        T = s["Tcw"][pose[0]][:3].reshape(-1) if len(pose) else np.eye(4, dtype=F32)[:3].reshape(-1)
        cam = s["cam"][pose[0]] if len(pose) else s["cam"][0]
        blob += [ids[k], float(k in spare), *cam, *T, len(keys[k]), len(cov) if k == cur else 0]
        for row in keys[k]:
            blob += list(row)
        if k == cur:
            blob += cov
    for m in range(n_mp):
        point = np.nonzero(mp_of_point == m)[0]
        X = s["Xw"][point[0]] if len(point) else (9.0, 9.0, 9.0)
        blob += [100 + m, float(m == bad_mp), *X, len(obs_of[m])]
        for row in obs_of[m]:
            blob += list(row)
    # what the gather produces: local poses (pKF, then its covisible ones that are not bad), points in
    # the order the local keyframes' match lists first show them, fixed poses in the order the points'
    # observations first show them, edges by point and inside by keyframe index
    point_order, seen = [], set()
    for p in local_order:
        for row in keys[kf_of_pose[p]]:
            m = int(row[4])
            if m >= 0 and m != bad_mp and m not in seen:
                seen.add(m)
                point_order.append(m)
    local_kfs = [int(kf_of_pose[p]) for p in local_order]
    fixed_kfs = []
    for m in point_order:
        for k, _ in sorted(obs_of[m]):
            if k not in local_kfs and k != bad_neighbour and k not in fixed_kfs and k != bad_observer:
                fixed_kfs.append(k)
    pose_kfs = local_kfs + fixed_kfs
    pose_of_kf = {k: i for i, k in enumerate(pose_kfs)}
    scene_pose = [int(np.nonzero(kf_of_pose == k)[0][0]) for k in pose_kfs]
    ep, el, ob, w = [], [], [], []
    for i, m in enumerate(point_order):
        for k, idx in sorted(obs_of[m]):
            if k in pose_of_kf:
                row = keys[k][idx]
                ep.append(pose_of_kf[k]), el.append(i)
                ob.append((row[0], row[1], row[3])), w.append(TABLE[int(row[2])])
    scene_point = [int(np.nonzero(mp_of_point == m)[0][0]) for m in point_order]
    fixed = np.array([1 if (i >= NL or s["fixed"][sp]) else 0 for i, sp in enumerate(scene_pose)], np.uint8)
    problem = dict(Tcw=s["Tcw"][scene_pose], fixed=fixed, cam=s["cam"][scene_pose],
                   Xw=s["Xw"][scene_point].reshape(-1, 3), pose_idx=np.array(ep, np.int32), point_idx=np.array(el, np.int32),
                   obs=np.array(ob, F32).reshape(-1, 3), inv_sigma2=np.array(w, F32), n_local=NL)
    bad_marked = with_points and any(int(m) in point_order for m in mp_of_point[:3])
    marks = dict(cur_id=int(ids[cur]), local=local_kfs + [bad_neighbour], fixed=fixed_kfs + ([bad_observer] if bad_marked else []),
                 points=point_order)
    return np.array(blob, np.float64), problem, pose_kfs, point_order, marks


def _run_adapter(exe, tmp_path, blob):
    (tmp_path / "scene.bin").write_bytes(np.asarray(blob, np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path / "scene.bin"), str(tmp_path / "out.txt")], check=True, timeout=120)
    return [line.split() for line in (tmp_path / "out.txt").read_text().split("\n") if line]


def _check_marks(lines, marks, n_kf, n_mp):
    """the mnBALocalForKF / mnBAFixedForKF bookkeeping of :545-592"""
    B = {int(l[1]): (int(l[2]), int(l[3])) for l in lines if l[0] == "B"}
    b = {int(l[1]): int(l[2]) for l in lines if l[0] == "b"}
    assert len(B) == n_kf and len(b) == n_mp
    cur = marks["cur_id"]
    if cur == 0:
        return  # the marks cannot be told from the initial zeros
    for k in range(n_kf):
        assert B[k] == (cur if k in marks["local"] else 0, cur if k in marks["fixed"] else 0), k
    for m in range(n_mp):
        assert b[m] == (cur if m in marks["points"] else 0), m


def test_adapter_builds_and_without_a_local_mappoint_touches_nothing(localba_main, tmp_path):
    """LocalBundleAdjuster.h compiles against the stand-ins with -Wall -Wextra -Werror; with no local
    MapPoint it needs no GPU and makes no call on a keyframe, a MapPoint or the map: only the
    bookkeeping marks of the local keyframes are set"""
    s = scene(**SIZES["p15"])
    blob, problem, pose_kfs, point_order, marks = _adapter_world(s, np.random.default_rng(5), with_points=False)
    assert len(problem["Xw"]) == 0 and len(problem["obs"]) == 0
    lines = _run_adapter(localba_main, tmp_path, blob)
    assert {l[0] for l in lines} == {"B", "b"}
    _check_marks(lines, marks, int(blob[0]), int(blob[1]))
    blob2, *_ = _adapter_world(s, np.random.default_rng(5))
    blob2[3] = 1.0  # *pbStopFlag set: the gather and its marks, then the return of :754-756
    assert {l[0] for l in _run_adapter(localba_main, tmp_path, blob2)} == {"B", "b"}


# ---------------------------------------------------------------- GPU

def _torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.gpu
def test_gpu_sizes_in_one_batch():
    _torch_gpu()
    scenes = [scene(**kw) for kw in SIZES.values()]
    refs = [ref(**kw) for kw in SIZES.values()]
    jobs, res, T, X, er = run_batch(scenes)
    worst = 0.0
    for k, (label, r) in enumerate(zip(SIZES, refs)):
        sp, sl, se = job_slices(jobs[k])
        worst = max(worst, check_against_ref(res[k], T[sp], X[sl], er[se], r, label))
    assert res["rounds"].tolist() == [0 if label == "e0" else 2 for label in SIZES]
    print(f"largest deviation of the size sweep: {worst:.3f} ulp")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases(name):
    """a far start with a rejected-then-accepted trial, a clean scene, a point and a local pose with
    every edge flagged, an edge flagged for its depth only, single-observation points, no fixed pose"""
    _torch_gpu()
    s, r = scene(**CASES[name]), ref(**CASES[name])
    jobs, res, T, X, er = run_batch([s])
    check_against_ref(res[0], T, X, er, r, name)
    T1, X1, e1, r1 = localba.local_bundle_adjustment(s["Tcw"], s["fixed"], s["cam"], s["Xw"], s["pose_idx"],
                                                     s["point_idx"], s["obs"], s["inv_sigma2"], s["n_local"])
    assert T1.tobytes() == T.tobytes() and X1.tobytes() == X.tobytes() and np.array_equal(e1, er.astype(bool))
    assert r1.tobytes() == res[0].tobytes()


def _mixed_scenes(count, seed0):
    shapes = [(1, 1, 1), (2, 1, 9), (3, 0, 17), (3, 2, 40), (6, 1, 33), (2, 3, 64), (4, 2, 65), (1, 0, 5)]
    out = []
    for k in range(count):
        nl, nfix, m = shapes[k % len(shapes)]
        out.append(synth.localba_scene(nl, nfix, m, seed0 + k, stereo=(0.0, 1.0, 0.4)[k % 3] if nfix else 1.0,
                                       outliers=0.1 if k % 4 == 1 else 0.0, kf0_local=(nfix == 0 and k % 2 == 0),
                                       **(dict(start_rot=0.15, start_t=0.5, start_pt=0.5) if k % 7 == 3 else {})))
    return out


@pytest.mark.gpu
def test_gpu_batch_invariance_and_determinism():
    """32 jobs of mixed shapes: each job alone gives the bytes it gives in the batch, at any position;
    a second batch call gives the same bytes"""
    _torch_gpu()
    scenes = _mixed_scenes(32, 700)
    jobs, res, T, X, er = run_batch(scenes)
    _, res2, T2, X2, er2 = run_batch(scenes)
    for a, b in ((res, res2), (T, T2), (X, X2), (er, er2)):
        assert a.tobytes() == b.tobytes()
    assert (res["rounds"] == 2).all() and (res["lm_iterations"] >= 1).all()
    for k, s in enumerate(scenes):
        _, r1, T1, X1, e1 = run_batch([s])
        sp, sl, se = job_slices(jobs[k])
        assert r1[0].tobytes() == res[k].tobytes() and T1.tobytes() == T[sp].tobytes(), k
        assert X1.tobytes() == X[sl].tobytes() and e1.tobytes() == er[se].tobytes(), k
    order = np.random.default_rng(1).permutation(len(scenes))
    jp, rp, Tp, Xp, ep = run_batch([scenes[k] for k in order])
    for pos, k in enumerate(order):
        a, b = job_slices(jp[pos]), job_slices(jobs[k])
        assert rp[pos].tobytes() == res[k].tobytes(), (pos, k)
        assert Tp[a[0]].tobytes() == T[b[0]].tobytes() and Xp[a[1]].tobytes() == X[b[1]].tobytes(), (pos, k)
        assert ep[a[2]].tobytes() == er[b[2]].tobytes(), (pos, k)


def _with_gaps(scenes, gap):
    """(jobs, input arrays) with `gap` unowned elements before, between and after the jobs' ranges
    in every array (unowned edges carry index -1: never read)"""
    jobs, _ = localba.make_batch(scenes)
    for k in range(len(jobs)):
        for name in ("pose_offset", "point_offset", "edge_offset", "out_pose_offset"):
            jobs[name][k] += gap * (k + 1)
    _, packed = localba.make_batch(scenes)
    arrays = {}
    for name, dtype, cols, kind in localba.INPUTS:
        count = {"poses": "n_poses", "points": "n_points", "edges": "n_edges"}[kind]
        fill = np.full((gap, cols) if cols else (gap,), -1 if name.startswith("edge_") else 0, dtype)
        parts, at = [fill], 0
        for j in jobs:
            parts += [packed[name][at:at + j[count]], fill]
            at += j[count]
        arrays[name] = np.concatenate(parts)
    return jobs, arrays


@pytest.mark.gpu
def test_gpu_nan_job_is_isolated_and_the_call_returns():
    """a job with a NaN in a local pose between two normal jobs, with gaps of unowned elements before,
    between and after the jobs in every array and guard bytes around every device array: the call
    returns, the neighbours' bytes equal those of a batch without the NaN job, every unowned element
    and every guard byte keeps its value, the inputs are not written"""
    torch = _torch_gpu()
    scenes = [dict(scene(**SIZES[n])) for n in ("p65", "e63", "e260")]
    gap, G = 5, 64
    jobs, arrays = _with_gaps(scenes, gap)
    tl = int(jobs["out_pose_offset"][-1] + jobs["n_local"][-1]) + gap
    tp, tm, te = len(arrays["Tcw"]), len(arrays["Xw"]), len(arrays["obs"])
    clean_res, clean_T, clean_X, clean_e = localba.local_ba_batch(
        jobs[[0, 2]], *(arrays[n] for n, *_ in localba.INPUTS), np.full((tl, 16), 7.5, F32), np.full((tm, 3), 7.5, F32),
        np.full(te, 0xA5, np.uint8), total_local=tl)
    arrays["Tcw"][jobs["pose_offset"][1] + 1, 5] = np.nan
    ML = int(jobs["n_local"].max())

    def guarded(a):
        flat = torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1).view(torch.uint8)
        full = torch.full((G + flat.numel() + G,), 0xC3, dtype=torch.uint8, device="cuda")
        full[G:G + flat.numel()] = flat
        view = full[G:G + flat.numel()].view(torch.from_numpy(a[:0]).dtype).reshape(a.shape)
        return full, view

    d_in = [guarded(arrays[n]) for n, *_ in localba.INPUTS]
    d_jobs = guarded(jobs.view(np.uint8).reshape(3, -1))
    outs = [guarded(np.full((tl, 16), 7.5, F32)), guarded(np.full((tm, 3), 7.5, F32)), guarded(np.full(te, 0xA5, np.uint8)),
            guarded(np.full((3, 32), 0x3C, np.uint8))]
    ws = guarded(np.zeros(localba.workspace_bytes(3, tp, tm, te, ML), np.uint8))
    before = [f.clone() for f, _ in d_in + [d_jobs]]
    localba.local_ba_batch_device(d_jobs[1], *(v for _, v in d_in), *(v for _, v in outs), ws[1], ML)
    torch.cuda.synchronize()
    for (f, _), b in zip(d_in + [d_jobs], before):
        assert torch.equal(f.view(torch.uint8), b.view(torch.uint8))
    for f, v in outs + [ws]:
        h = f.cpu().numpy()
        assert (h[:G] == 0xC3).all() and (h[-G:] == 0xC3).all()
    T, X, er = (v.cpu().numpy() for _, v in outs[:3])
    got = outs[3][1].cpu().numpy().reshape(-1).view(localba.RESULT_DTYPE)
    assert got[0].tobytes() == clean_res[0].tobytes() and got[2].tobytes() == clean_res[1].tobytes()
    owned = [np.zeros(n, bool) for n in (tl, tm, te)]
    for k in (0, 2):
        for own, sl, a, b in zip(owned, job_slices(jobs[k]), (T, X, er), (clean_T, clean_X, clean_e)):
            own[sl] = True
            assert a[sl].tobytes() == b[sl].tobytes(), k
    nan_slices = job_slices(jobs[1])
    for own, sl in zip(owned, nan_slices):
        own[sl] = True
    assert (T[~owned[0]] == F32(7.5)).all() and (X[~owned[1]] == F32(7.5)).all() and (er[~owned[2]] == 0xA5).all()
    assert got[1]["rounds"] == 2 and (got[1]["lm_iterations"] <= [5, 10]).all()
    assert set(np.unique(er[nan_slices[2]])) <= {0, 1}


@pytest.mark.gpu
def test_gpu_device_form_on_a_stream():
    """torch tensors on a non-default stream, read after stream.synchronize(); a job with an edge
    index out of range and one with a range beyond the totals (which the device form cannot check on
    the host) get rounds = -1 and write nothing else"""
    torch = _torch_gpu()
    labels = ["p65", "e255", "p17_kf0", "e65"]
    scenes, refs = [dict(scene(**SIZES[n])) for n in labels], [ref(**SIZES[n]) for n in labels]
    jobs, a = localba.make_batch(scenes)
    a["edge_pose"][jobs["edge_offset"][3] + 7] = jobs["n_poses"][3]  # job 3: one past its last pose
    bad = jobs[:1].copy()
    bad["edge_offset"] = len(a["obs"]) - 5
    jobs = np.concatenate([jobs, bad])
    tl, tm, te = int(jobs["n_local"][:4].sum()), len(a["Xw"]), len(a["obs"])
    ML = int(jobs["n_local"].max())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(len(jobs), -1)).cuda()
        d_in = [torch.from_numpy(np.ascontiguousarray(a[n])).cuda() for n, *_ in localba.INPUTS]
        d_T = torch.full((tl, 16), 7.5, dtype=torch.float32, device="cuda")
        d_X = torch.full((tm, 3), 7.5, dtype=torch.float32, device="cuda")
        d_e = torch.full((te,), 9, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((len(jobs), 32), dtype=torch.uint8, device="cuda")
        d_ws = torch.empty(localba.workspace_bytes(len(jobs), len(a["Tcw"]), tm, te, ML), dtype=torch.uint8, device="cuda")
    localba.local_ba_batch_device(d_jobs, *d_in, d_T, d_X, d_e, d_res, d_ws, ML, stream=st)
    st.synchronize()
    res = d_res.cpu().numpy().reshape(-1).view(localba.RESULT_DTYPE)
    T, X, er = d_T.cpu().numpy(), d_X.cpu().numpy(), d_e.cpu().numpy()
    for k in range(3):
        sp, sl, se = job_slices(jobs[k])
        check_against_ref(res[k], T[sp], X[sl], er[se], refs[k], labels[k])
    assert res["rounds"].tolist() == [2, 2, 2, -1, -1]
    sp, sl, se = job_slices(jobs[3])
    assert (T[sp] == F32(7.5)).all() and (X[sl] == F32(7.5)).all() and (er[se] == 9).all()


@pytest.mark.gpu
def test_gpu_device_form_on_a_second_device():
    torch = _torch_gpu()
    n = orbgpu.device_count()
    if n < 2:
        pytest.skip(f"{n} visible device(s): the second-device call needs >= 2")
    s, r = scene(**SIZES["e255"]), ref(**SIZES["e255"])
    jobs, a = localba.make_batch([s])
    prev = orbgpu.get_thread_device()
    try:
        orbgpu.set_thread_device(1)
        with torch.cuda.device(1):
            dev = torch.device("cuda", 1)
            t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                 for v in (jobs.view(np.uint8).reshape(1, -1), *(a[n] for n, *_ in localba.INPUTS))]
            NL, M, E = int(jobs["n_local"][0]), len(a["Xw"]), len(a["obs"])
            d_T = torch.zeros((NL, 16), dtype=torch.float32, device=dev)
            d_X = torch.zeros((M, 3), dtype=torch.float32, device=dev)
            d_e = torch.zeros(E, dtype=torch.uint8, device=dev)
            d_res = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
            d_ws = torch.empty(localba.workspace_bytes(1, len(a["Tcw"]), M, E, NL), dtype=torch.uint8, device=dev)
            localba.local_ba_batch_device(*t, d_T, d_X, d_e, d_res, d_ws, NL, stream=torch.cuda.current_stream(dev))
            torch.cuda.synchronize(dev)
            res = d_res.cpu().numpy().reshape(-1).view(localba.RESULT_DTYPE)
            check_against_ref(res[0], d_T.cpu().numpy(), d_X.cpu().numpy(), d_e.cpu().numpy(), r, "e255")
    finally:
        orbgpu.set_thread_device(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p65", "p17_kf0"])
def test_gpu_adapter(localba_main, tmp_path, name):
    """LocalBundleAdjustmentGPU on stand-in keyframes with bad keyframes, bad and null MapPoints and
    (p17_kf0) keyframe 0 interleaved: the erased observations in the reference's order (monocular
    edges, then stereo), every SetPose and SetWorldPos value, the call order and the bookkeeping
    marks, against the restatement run on what the gather must produce"""
    _torch_gpu()
    s = scene(**SIZES[name])
    blob, problem, pose_kfs, point_order, marks = _adapter_world(s, np.random.default_rng(3))
    r = localba_ref.run_scene(problem)
    check_margins(r, problem, name)
    lines = _run_adapter(localba_main, tmp_path, blob)
    calls = [l for l in lines if l[0] not in "Bb"]
    stereo = problem["obs"][:, 2] >= 0
    erased = [e for e in np.nonzero(r.erase & ~stereo)[0]] + [e for e in np.nonzero(r.erase & stereo)[0]]
    if name == "p65":
        assert len(erased) > 0 and (r.erase & stereo).any() and (r.erase & ~stereo).any()
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
    assert dev <= ULP_BOUND
    _check_marks(lines, marks, int(blob[0]), int(blob[1]))
