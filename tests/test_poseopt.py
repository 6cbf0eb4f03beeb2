"""Motion-only pose optimisation (include/orbgpu_poseopt.h, csrc/poseopt.hip,
include/orbslam2_amd/PoseOptimizer.h) against the numpy restatement of
Optimizer::PoseOptimization (tests/poseopt_ref.py).

Parity: every element of the float32 pose within 2 float32 ulps at the scale
max(1, max|Tcw|) -- one for a double that sits on a float rounding boundary,
one of slack; outlier flags, n_good and rounds equal.  The kernel and the
oracle add the edges in different orders, so the LM traces are not compared
(at convergence accept / reject is decided by rounding noise): lm_iterations is
only checked for its range.  Every scene's seed is fixed and, in the oracle,
keeps every classification chi2 of every round at least 1e-6 (relative) away
from its threshold; the tests assert that on the CPU before they compare.
"""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orbgpu
import poseopt
import poseopt_ref
import synth

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32
ULP = 2.0 ** -23
MARGIN = 1e-6

# n of the size sweep -> seed: the wave (64) and workgroup (256) boundaries, more than one
# edge per lane, the n < 3 and n < 10 rules, and 4100 edges: past the 1536 the kernel keeps in LDS
SIZE_SEEDS = {0: 100, 2: 102, 3: 103, 9: 109, 10: 110, 63: 163, 64: 164, 65: 165, 255: 1255, 256: 1256, 257: 1257,
              1030: 2030, 4100: 5100}
FAR = dict(start_rot=0.5, start_t=0.8)
# A start whose oracle trace has, in every round, a rejected trial followed by an accepted one
# that still lowers the robust chi2 by more than 1 %.  Found by searching seeds with the oracle:
# none of 600 seeds at 0.5 rad / 0.8 m shows one, seed 208 at 1.3 rad / 2 m does.
FAR_REJECT = dict(n=300, seed=208, start_rot=1.3, start_t=2.0)
CASES = {
    "mono": dict(n=300, seed=11, stereo=0.0),
    "stereo": dict(n=300, seed=12, stereo=1.0),
    "far": dict(n=300, seed=13, **FAR),
    "far_reject": FAR_REJECT,
    "behind": dict(n=65, seed=14, behind=1),
}


@functools.lru_cache(maxsize=None)
def _scene_cached(items):
    kw = dict(items)
    s = synth.pose_scene(kw.pop("n"), kw.pop("seed"), **kw)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def scene(**kw):
    return _scene_cached(tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _oracle_cached(items):
    s = _scene_cached(items)
    return poseopt_ref.pose_optimization(s["Tcw0"], s["Xw"], s["obs"], s["inv_sigma2"], s["K"], s["bf"])


def oracle(**kw):
    """the oracle's result of a scene, computed once per session, with the margin precondition"""
    r = _oracle_cached(tuple(sorted(kw.items())))
    assert poseopt_ref.threshold_margin(r, scene(**kw)["obs"]) >= MARGIN, kw
    return r


def size_scene(n):
    return dict(n=n, seed=SIZE_SEEDS[n])


def pack(scenes):
    """(jobs, Xw, obs, inv_sigma2) of a list of scenes laid out back to back"""
    frames, off = [], 0
    for s in scenes:
        frames.append((len(s["Xw"]), off, s["Tcw0"], s["K"], s["bf"]))
        off += len(s["Xw"])
    cat = lambda k, w: np.concatenate([s[k].reshape(-1, w) for s in scenes]) if scenes else np.zeros((0, w), F32)
    return poseopt.make_jobs(frames), cat("Xw", 3), cat("obs", 3), cat("inv_sigma2", 1).reshape(-1)


def check_against_oracle(res, flags, ref, label):
    """one job's RESULT_DTYPE record and flag bytes against the oracle; returns the pose deviation in ulps"""
    T = res["Tcw"].reshape(4, 4)
    scale = max(1.0, float(np.abs(ref.Tcw).max()))
    dev = float(np.abs(T.astype(np.float64) - ref.Tcw.astype(np.float64)).max()) / (ULP * scale)
    print(f"{label}: pose deviation {dev:.3f} ulp, n_good {res['n_good']}, rounds {res['rounds']}, "
          f"iterations {list(res['lm_iterations'])}, rejected {list(res['lm_rejected'])}; oracle "
          f"{[(t.iterations, t.rejected) for t in ref.trace]}")
    assert np.array_equal(flags.astype(bool), ref.outlier), (label, int((flags.astype(bool) != ref.outlier).sum()))
    assert int(res["n_good"]) == ref.n_good and int(res["rounds"]) == ref.rounds, label
    assert dev <= 2.0, (label, dev)
    for k in range(4):
        if k < ref.rounds:
            assert 1 <= res["lm_iterations"][k] <= 10 and 0 <= res["lm_rejected"][k] <= 100, label
        else:
            assert res["lm_iterations"][k] == 0 and res["lm_rejected"][k] == 0, label
    assert tuple(T[3]) == (0.0, 0.0, 0.0, 1.0), label
    return dev


# ---------------------------------------------------------------- CPU: the oracle's own checks

def _random_edges(rng, n=40):
    s = synth.pose_scene(n, int(rng.integers(1 << 30)))
    est = poseopt_ref.se3_from_T(s["Tcw0"])
    K = tuple(float(F32(v)) for v in s["K"])
    return s, est, K, float(F32(s["bf"]))


def test_ref_jacobians_agree_with_central_differences():
    """d e / d x of e(exp(x) * est) at x = 0 is J (of the error obs - projection).  The stereo
    edge's float invz makes its error a step function at the 6e-8 relative level, so the
    differences are taken of the same error with invz kept in double (float_invz=False): one
    tolerance for both edge types, the O(h^2) truncation of the central difference."""
    rng = np.random.default_rng(5)
    s, est, K, bf = _random_edges(rng)
    Xw, obs, w = s["Xw"], s["obs"], s["inv_sigma2"].astype(np.float64)
    stereo = obs[:, 2] >= 0
    _, _, p = poseopt_ref.edge_errors(est, Xw, obs, w, K, bf)
    J = poseopt_ref.edge_jacobians(p, stereo, K, bf)
    h = 1e-4
    for j in range(6):
        d = [0.0] * 6
        d[j] = h
        ep, _, _ = poseopt_ref.edge_errors(poseopt_ref.se3_mul(poseopt_ref.se3_exp(d), est), Xw, obs, w, K, bf,
                                           float_invz=False)
        d[j] = -h
        em, _, _ = poseopt_ref.edge_errors(poseopt_ref.se3_mul(poseopt_ref.se3_exp(d), est), Xw, obs, w, K, bf,
                                           float_invz=False)
        num = (ep - em) / (2 * h)
        assert (np.abs(num - J[:, :, j]) <= 1e-4 * (1 + np.abs(J[:, :, j]))).all(), j
    assert stereo.sum() > 5 and (~stereo).sum() > 5
    assert np.abs(J[~stereo, 2]).max() == 0
    # a stereo edge's third row: zero in column 4 only (x or y = 0 does not occur in the scene)
    assert (J[stereo, 2][:, [0, 1, 2, 3, 5]] != 0).all() and (J[stereo, 2, 4] == 0).all()
    # the float invz moves the error by at most half a float ulp of invz: 6e-8 of ~700 px
    ef, _, _ = poseopt_ref.edge_errors(est, Xw, obs, w, K, bf)
    ed, _, _ = poseopt_ref.edge_errors(est, Xw, obs, w, K, bf, float_invz=False)
    assert np.array_equal(ef[~stereo], ed[~stereo]) and (ef[stereo] != ed[stereo]).any()
    assert np.abs(ef - ed).max() <= 700 * 2.0 ** -24 * 1.01


def test_ref_exp_returns_a_rotation():
    rng = np.random.default_rng(6)
    for scale in (1e-7, 1e-3, 0.3, 2.5):
        x = list(rng.normal(size=6) * scale)
        q, t = poseopt_ref.se3_exp(x)
        R = np.array(poseopt_ref.quat_to_R(q))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        th = np.linalg.norm(x[:3])
        assert th < 2 * np.pi
        assert abs(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)) - min(th, 2 * np.pi - th)) < 1e-7
        assert np.abs(np.array(t) - np.array(x[3:])).max() <= 2 * th * np.linalg.norm(x[3:]) + 1e-15
    q, t = poseopt_ref.se3_exp([0.0] * 6)
    assert q == [0.0, 0.0, 0.0, 1.0] and t == [0.0, 0.0, 0.0]


def test_ref_noise_free_flags_exactly_the_injected_outliers():
    for seed, n in ((21, 120), (22, 300)):
        s = synth.pose_scene(n, seed, noise=0.0, outliers=0.2)
        r = poseopt_ref.pose_optimization(s["Tcw0"], s["Xw"], s["obs"], s["inv_sigma2"], s["K"], s["bf"])
        assert s["outlier"].sum() > 10 and np.array_equal(r.outlier, s["outlier"])
        assert r.n_good == n - s["outlier"].sum() and r.rounds == 4

        def cost(T):
            _, chi2, _ = poseopt_ref.edge_errors(poseopt_ref.se3_from_T(T), s["Xw"], s["obs"],
                                                 s["inv_sigma2"].astype(np.float64),
                                                 tuple(float(F32(v)) for v in s["K"]), float(F32(s["bf"])))
            return chi2[~s["outlier"]].sum()
        assert cost(r.Tcw) < 1e-3 * cost(s["Tcw0"])


def test_ref_rules_for_few_observations():
    s = synth.pose_scene(2, 31)
    r = poseopt_ref.pose_optimization(s["Tcw0"], s["Xw"], s["obs"], s["inv_sigma2"], s["K"], s["bf"])
    assert r.n_good == 0 and r.rounds == 0 and not r.outlier.any() and r.Tcw.tobytes() == s["Tcw0"].tobytes()
    s = synth.pose_scene(9, 32)
    r = poseopt_ref.pose_optimization(s["Tcw0"], s["Xw"], s["obs"], s["inv_sigma2"], s["K"], s["bf"])
    assert r.rounds == 1 and len(r.trace) == 1


@pytest.mark.parametrize("seed,n,kw", [(41, 120, {}), (42, 300, {}), (43, 300, FAR), (44, 1030, {})])
def test_ref_is_stable_under_a_permutation_of_the_observations(seed, n, kw):
    """the same scene with its observations permuted (every sum rounds differently): the float32
    pose within the GPU tests' bound, the flags equal"""
    s = synth.pose_scene(n, seed, **kw)
    a = poseopt_ref.pose_optimization(s["Tcw0"], s["Xw"], s["obs"], s["inv_sigma2"], s["K"], s["bf"])
    assert poseopt_ref.threshold_margin(a, s["obs"]) >= MARGIN
    p = np.random.default_rng(seed).permutation(n)
    b = poseopt_ref.pose_optimization(s["Tcw0"], s["Xw"][p], s["obs"][p], s["inv_sigma2"][p], s["K"], s["bf"])
    assert np.array_equal(a.outlier[p], b.outlier) and a.n_good == b.n_good
    scale = max(1.0, float(np.abs(a.Tcw).max()))
    assert np.abs(a.Tcw.astype(np.float64) - b.Tcw).max() <= 2 * ULP * scale


def test_scene_preconditions():
    """every fixed scene keeps its classification chi2 away from the thresholds; the far-start
    fixture's trace has a rejected trial followed by an accepted one before convergence; the
    behind-the-camera scene has its point behind the camera at the start and at the end"""
    for n in SIZE_SEEDS:
        r = oracle(**size_scene(n))
        assert r.rounds == (0 if n < 3 else 1 if n < 10 else 4)
    for name, kw in CASES.items():
        r = oracle(**kw)
        assert r.rounds == 4 and 0 < r.outlier.sum() < kw["n"], name
    assert not (scene(**CASES["mono"])["obs"][:, 2] >= 0).any() and (scene(**CASES["stereo"])["obs"][:, 2] >= 0).all()
    s = scene(**size_scene(1030))
    assert 0.3 < (s["obs"][:, 2] >= 0).mean() < 0.7 and 0.1 < s["outlier"].mean() < 0.3
    found = False
    for tr in oracle(**CASES["far_reject"]).trace:
        for k in range(1, len(tr.trials)):
            if not tr.trials[k - 1] and tr.trials[k] and tr.chi_after[k] < 0.99 * tr.chi_after[k - 1]:
                found = True
    assert found
    s = scene(**CASES["behind"])
    for T in (s["Tcw0"], oracle(**CASES["behind"]).Tcw):
        z = (s["Xw"].astype(np.float64) @ T[2, :3].astype(np.float64)) + T[2, 3]
        assert z[0] < 0 and (z[1:] > 0).all()


# ---------------------------------------------------------------- CPU: argument checks of the library

def _args(form, **kw):
    jobs = poseopt.make_jobs([(4, 0, np.eye(4), (500, 500, 320, 240), 40.0), (6, 4, np.eye(4), (500, 500, 320, 240), 40.0)])
    a = dict(batch=2, jobs=jobs, total=10, Xw=1 << 12, obs=1 << 13, w=1 << 14, res=1 << 15, out=1 << 16)
    a.update(kw)
    jobs = a["jobs"]
    jp = None if jobs is None else (jobs.ctypes.data if form == "host" else 1 << 17)
    L = orbgpu.lib()
    if form == "host":
        return L.orbgpu_pose_optimization_batch(a["batch"], jp, a["total"], a["Xw"], a["obs"], a["w"], a["res"],
                                                a["out"])
    return L.orbgpu_pose_optimization_batch_device(a["batch"], jp, a["total"], a["Xw"], a["obs"], a["w"], a["res"],
                                                   a["out"], None)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_checks_need_no_device(form):
    """rejected on the host before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    assert _args(form, batch=-1) == E and _args(form, total=-1) == E
    for name in ("jobs", "Xw", "obs", "w", "res", "out"):
        assert _args(form, **{name: None}) == E, name
    assert "null" in orbgpu.last_error()
    assert _args(form, batch=0) == orbgpu.OK
    assert _args(form, batch=0, total=0, jobs=None, Xw=None, obs=None, w=None, res=None, out=None) == orbgpu.OK


def test_job_range_checks_need_no_device():
    E = orbgpu.ERR_ARG

    def jobs(n0, off0, n1=6, off1=4):
        I, K = np.eye(4), (500, 500, 320, 240)
        return poseopt.make_jobs([(n0, off0, I, K, 40.0), (n1, off1, I, K, 40.0)])
    assert _args("host", jobs=jobs(-1, 0)) == E
    assert "job 0" in orbgpu.last_error()
    assert _args("host", jobs=jobs(4, -1)) == E
    assert _args("host", jobs=jobs(4, 0, 7, 4)) == E  # 4 + 7 > 10
    assert "job 1" in orbgpu.last_error()
    assert _args("host", jobs=jobs(4, 0, 1, 10)) == E
    assert _args("host", jobs=jobs(4, 0, 2 ** 31 - 1, 2 ** 31 - 1)) == E  # the sum does not wrap
    # total_obs == 0: every job is empty; the host writes the results, nothing is launched
    j = jobs(0, 0, 0, 0)
    j["Tcw0"][1] = np.arange(12)
    res = np.full(2 * poseopt.RESULT_DTYPE.itemsize, 0x5A, np.uint8).view(poseopt.RESULT_DTYPE)
    assert _args("host", jobs=j, total=0, Xw=None, obs=None, w=None, out=None, res=res.ctypes.data) == orbgpu.OK
    assert res["n_good"].tolist() == [0, 0] and res["rounds"].tolist() == [0, 0]
    assert not res["lm_iterations"].any() and not res["lm_rejected"].any()
    assert res["Tcw"][1].tolist() == list(range(12)) + [0, 0, 0, 1]
    assert _args("host", jobs=jobs(1, 0, 0, 0), total=0, Xw=None, obs=None, w=None, out=None) == E


def test_python_wrapper_and_struct_layout():
    assert ctypes.sizeof(poseopt.PoseOptJob) == 80 and ctypes.sizeof(poseopt.PoseOptResult) == 104
    assert poseopt.PoseOptResult.Tcw.offset == poseopt.RESULT_DTYPE.fields["Tcw"][1] == 40
    assert poseopt.PoseOptJob.fx.offset == poseopt.JOB_DTYPE.fields["fx"][1] == 56
    with pytest.raises(ValueError):
        poseopt.pose_optimization_batch(poseopt.make_jobs([]), np.zeros((3, 3)), np.zeros((2, 3)), np.zeros(3))
    with pytest.raises(ValueError):
        poseopt.pose_optimization_batch(poseopt.make_jobs([]), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3),
                                        outlier=np.zeros(3, np.int32))
    res, out = poseopt.pose_optimization_batch(poseopt.make_jobs([]), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
    assert len(res) == 0 and len(out) == 0
    T, out, n_good = poseopt.pose_optimization(np.eye(4), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0),
                                               (500, 500, 320, 240), 40.0)
    assert T.tobytes() == np.eye(4, dtype=F32).tobytes() and len(out) == 0 and n_good == 0


# ---------------------------------------------------------------- the C++ adapter

@pytest.fixture(scope="module")
def poseopt_main(tmp_path_factory):
    """tests/cpp/poseopt_main.cpp against PoseOptimizer.h and the cvlite stand-ins, one g++ line"""
    pkg = ROOT / "orb-slam2-annotation_amd"
    exe = tmp_path_factory.mktemp("poseopt") / "poseopt_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'tests' / 'cpp'}", '-DORBGPU_CV_HEADER="cvlite.hpp"', "-pthread", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "poseopt_main.cpp"), f"-L{pkg}", "-lorbgpu", f"-Wl,-rpath,{pkg}"],
                   check=True)
    return exe


def _run_adapter(exe, tmp_path, s, has_mp, preset):
    """the scene's observations placed at the keypoints with has_mp, junk elsewhere"""
    N = len(has_mp)
    rows = np.zeros((N, 9), F32)
    rows[:, 0] = has_mp
    idx = np.nonzero(has_mp)[0]
    assert len(idx) == len(s["Xw"])
    rows[:, 1:4] = 1e3  # a keypoint without a MapPoint must not be read as an observation
    rows[:, 4:7] = (50.0, 60.0, -1.0)
    rows[idx, 1:4], rows[idx, 4:7] = s["Xw"], s["obs"]
    octave = np.rint(np.log(1.0 / s["inv_sigma2"].astype(np.float64)) / (2 * np.log(1.2))).astype(int)
    table = (1.0 / 1.2 ** (2.0 * np.arange(8))).astype(F32)
    assert np.array_equal(table[octave], s["inv_sigma2"])
    rows[idx, 7] = octave
    rows[:, 8] = preset
    T0 = np.eye(4, dtype=F32)
    T0[:3] = s["Tcw0"][:3]
    blob = np.concatenate([[F32(N)], T0.reshape(-1), np.array([*s["K"], s["bf"]], F32), table, rows.reshape(-1)])
    (tmp_path / "scene.bin").write_bytes(blob.astype(F32).tobytes())
    subprocess.run([str(exe), str(tmp_path / "scene.bin"), str(tmp_path / "out.txt")], check=True, timeout=120)
    lines = (tmp_path / "out.txt").read_text().split("\n")
    ret, calls = (int(v) for v in lines[0].split())
    T = np.array([int(v, 16) for v in lines[1].split()], np.uint32).view(F32).reshape(4, 4)
    return ret, calls, T, np.array([c == "1" for c in lines[2].strip()], bool), idx


def test_adapter_builds_and_handles_an_empty_frame(poseopt_main, tmp_path):
    """PoseOptimizer.h compiles against the stand-ins; a frame without MapPoints needs no GPU:
    returns 0, SetPose is not called, mvbOutlier keeps its preset"""
    s = synth.pose_scene(0, 1)
    preset = np.array([1, 0, 1, 1, 0], bool)
    ret, calls, T, flags, _ = _run_adapter(poseopt_main, tmp_path, s, np.zeros(5, bool), preset)
    assert (ret, calls) == (0, 0) and np.array_equal(flags, preset)
    assert T[:3].tobytes() == s["Tcw0"][:3].tobytes()


# ---------------------------------------------------------------- GPU

def _torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.gpu
def test_gpu_sizes_in_one_batch():
    _torch_gpu()
    kws = [size_scene(n) for n in SIZE_SEEDS]
    refs = [oracle(**kw) for kw in kws]
    jobs, Xw, obs, w = pack([scene(**kw) for kw in kws])
    res, out = poseopt.pose_optimization_batch(jobs, Xw, obs, w, np.full(len(Xw), 0xA5, np.uint8))
    worst = 0.0
    for k, (j, kw, ref) in enumerate(zip(jobs, kws, refs)):
        sl = slice(j["offset"], j["offset"] + j["n"])
        worst = max(worst, check_against_oracle(res[k], out[sl], ref, f"n={kw['n']}"))
    assert res["Tcw"][0].reshape(4, 4)[:3].tobytes() == scene(**kws[0])["Tcw0"][:3].tobytes()  # n = 0, 2: untouched
    assert res["Tcw"][1].reshape(4, 4)[:3].tobytes() == scene(**kws[1])["Tcw0"][:3].tobytes()
    print(f"largest pose deviation of the size sweep: {worst:.3f} ulp")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases(name):
    """all-monocular, all-stereo, far start (0.5 rad, 0.8 m), a start with a rejected-then-
    accepted trial, one point behind the camera in a job of 65"""
    _torch_gpu()
    s, ref = scene(**CASES[name]), oracle(**CASES[name])
    T, out, n_good = poseopt.pose_optimization(s["Tcw0"], s["Xw"], s["obs"], s["inv_sigma2"], s["K"], s["bf"])
    jobs, Xw, obs, w = pack([s])
    res, flags = poseopt.pose_optimization_batch(jobs, Xw, obs, w)
    check_against_oracle(res[0], flags, ref, name)
    assert T.tobytes() == res["Tcw"][0].tobytes() and np.array_equal(out, flags.astype(bool)) and n_good == ref.n_good


def _mixed_scenes(count, seed0):
    sizes = [5, 40, 64, 65, 130, 256, 300, 700, 1030, 1600]
    return [synth.pose_scene(sizes[k % len(sizes)], seed0 + k, stereo=(0.5, 0.0, 1.0)[k % 3],
                             **(FAR if k % 7 == 3 else {})) for k in range(count)]


@pytest.mark.gpu
def test_gpu_batch_invariance_and_determinism():
    """64 jobs of mixed sizes: each job alone gives the bytes it gives in the batch, at any
    position; a second batch call gives the same bytes"""
    _torch_gpu()
    scenes = _mixed_scenes(64, 700)
    jobs, Xw, obs, w = pack(scenes)
    res, out = poseopt.pose_optimization_batch(jobs, Xw, obs, w)
    res2, out2 = poseopt.pose_optimization_batch(jobs, Xw, obs, w)
    assert res.tobytes() == res2.tobytes() and out.tobytes() == out2.tobytes()
    assert (res["rounds"] == np.where(jobs["n"] < 10, 1, 4)).all()
    big = jobs["n"] >= 40
    assert (res["n_good"][big] > 0.5 * jobs["n"][big]).all() and (res["n_good"][big] < jobs["n"][big]).all()
    for k, s in enumerate(scenes):
        j1, X1, o1, w1 = pack([s])
        r1, f1 = poseopt.pose_optimization_batch(j1, X1, o1, w1)
        sl = slice(jobs["offset"][k], jobs["offset"][k] + jobs["n"][k])
        assert r1[0].tobytes() == res[k].tobytes() and f1.tobytes() == out[sl].tobytes(), k
    order = np.random.default_rng(1).permutation(64)
    jp, Xp, op, wp = pack([scenes[k] for k in order])
    rp, fp = poseopt.pose_optimization_batch(jp, Xp, op, wp)
    for pos, k in enumerate(order):
        assert rp[pos].tobytes() == res[k].tobytes(), (pos, k)


@pytest.mark.gpu
def test_gpu_nan_job_is_isolated_and_the_call_returns():
    """a job whose Tcw0 holds a NaN between two normal jobs, with a gap of unowned observations
    before, between and after the jobs: the neighbours' bytes equal those of a batch without it,
    unowned flag bytes and the guard bytes around the device arrays keep their values"""
    torch = _torch_gpu()
    a, b, c = (synth.pose_scene(n, seed) for n, seed in ((300, 801), (200, 802), (257, 803)))
    gap = 7
    frames, off, Xs, os_, ws = [], gap, [], [], []
    for s in (a, b, c):
        n = len(s["Xw"])
        frames.append((n, off, s["Tcw0"], s["K"], s["bf"]))
        off += n + gap
        for lst, k, wd in ((Xs, "Xw", 3), (os_, "obs", 3), (ws, "inv_sigma2", 1)):
            lst += [np.zeros((gap, wd), F32), s[k].reshape(-1, wd)]
    total = off
    Xw, obs, w = (np.concatenate(l + [np.zeros((gap, l[0].shape[1]), F32)]) for l in (Xs, os_, ws))
    w = w.reshape(-1)
    assert len(Xw) == total
    jobs = poseopt.make_jobs(frames)
    clean, clean_out = poseopt.pose_optimization_batch(jobs[[0, 2]], Xw, obs, w, np.full(total, 0xA5, np.uint8))
    jobs["Tcw0"][1][5] = np.nan
    G = 64
    d = {k: torch.from_numpy(v).cuda() for k, v in (("jobs", jobs.view(np.uint8).reshape(3, -1)), ("Xw", Xw),
                                                    ("obs", obs), ("w", w))}
    res = torch.full((G + 3 * 104 + G,), 0xC3, dtype=torch.uint8, device="cuda")
    out = torch.full((G + total + G,), 0xA5, dtype=torch.uint8, device="cuda")
    poseopt.pose_optimization_batch_device(d["jobs"], d["Xw"], d["obs"], d["w"], res[G:G + 312].view(3, 104),
                                           out[G:G + total])
    torch.cuda.synchronize()
    res_h, out_h = res.cpu().numpy(), out.cpu().numpy()
    assert (res_h[:G] == 0xC3).all() and (res_h[-G:] == 0xC3).all()
    assert (out_h[:G] == 0xA5).all() and (out_h[-G:] == 0xA5).all()
    got = res_h[G:G + 312].view(poseopt.RESULT_DTYPE)
    flags = out_h[G:G + total]
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[1].tobytes()
    owned = np.zeros(total, bool)
    for k in (0, 2):
        sl = slice(jobs["offset"][k], jobs["offset"][k] + jobs["n"][k])
        owned[sl] = True
        assert flags[sl].tobytes() == clean_out[sl].tobytes()
        assert set(np.unique(flags[sl])) <= {0, 1}
    owned[jobs["offset"][1]:jobs["offset"][1] + jobs["n"][1]] = True
    assert (flags[~owned] == 0xA5).all()
    owned[jobs["offset"][1]:jobs["offset"][1] + jobs["n"][1]] = False
    assert (clean_out[~owned] == 0xA5).all()
    assert got[1]["rounds"] == 4 and (got[1]["lm_iterations"] >= 1).all() and (got[1]["lm_iterations"] <= 10).all()


@pytest.mark.gpu
def test_gpu_device_form_on_a_stream():
    """torch tensors on a non-default stream, read after stream.synchronize(); a job with an
    out-of-range offset (which the device form cannot check on the host) gets rounds = -1"""
    torch = _torch_gpu()
    kws = [size_scene(257), CASES["stereo"], size_scene(9)]
    scenes, refs = [scene(**kw) for kw in kws], [oracle(**kw) for kw in kws]
    jobs, Xw, obs, w = pack(scenes)
    bad = jobs[:1].copy()
    bad["offset"] = len(Xw) - 5
    jobs = np.concatenate([jobs, bad])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(len(jobs), -1)).cuda()
        d_X, d_o, d_w = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Xw, obs, w))
        d_res = torch.zeros((len(jobs), 104), dtype=torch.uint8, device="cuda")
        d_out = torch.full((len(Xw),), 9, dtype=torch.uint8, device="cuda")
    poseopt.pose_optimization_batch_device(d_jobs, d_X, d_o, d_w, d_res, d_out, stream=s)
    s.synchronize()
    res = d_res.cpu().numpy().reshape(-1).view(poseopt.RESULT_DTYPE)
    out = d_out.cpu().numpy()
    for k, ref in enumerate(refs):
        check_against_oracle(res[k], out[jobs["offset"][k]:jobs["offset"][k] + jobs["n"][k]], ref, f"job {k}")
    assert res[3]["rounds"] == -1 and res[3]["n_good"] == -1


@pytest.mark.gpu
def test_gpu_device_form_on_a_second_device():
    torch = _torch_gpu()
    n = orbgpu.device_count()
    if n < 2:
        pytest.skip(f"{n} visible device(s): the second-device call needs >= 2")
    kw = size_scene(257)
    jobs, Xw, obs, w = pack([scene(**kw)])
    prev = orbgpu.get_thread_device()
    try:
        orbgpu.set_thread_device(1)
        with torch.cuda.device(1):
            dev = torch.device("cuda", 1)
            t = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (jobs.view(np.uint8).reshape(1, -1), Xw,
                                                                             obs, w)]
            d_res = torch.zeros((1, 104), dtype=torch.uint8, device=dev)
            d_out = torch.zeros(len(Xw), dtype=torch.uint8, device=dev)
            poseopt.pose_optimization_batch_device(*t, d_res, d_out, stream=torch.cuda.current_stream(dev))
            torch.cuda.synchronize(dev)
            res = d_res.cpu().numpy().reshape(-1).view(poseopt.RESULT_DTYPE)
            check_against_oracle(res[0], d_out.cpu().numpy(), oracle(**kw), "device 1")
    finally:
        orbgpu.set_thread_device(prev)


@pytest.mark.gpu
def test_gpu_adapter(poseopt_main, tmp_path):
    """PoseOptimizationGPU on a stand-in Frame with null MapPoints interleaved: mvbOutlier at
    keypoints without a MapPoint keeps its preset, pose / flags / return value equal the
    oracle's; a frame with two MapPoints returns 0 without SetPose and clears their flags"""
    _torch_gpu()
    kw = size_scene(255)
    s, ref = scene(**kw), oracle(**kw)
    rng = np.random.default_rng(3)
    N = 400
    has_mp = np.zeros(N, bool)
    has_mp[np.sort(rng.choice(N, 255, replace=False))] = True
    preset = rng.random(N) < 0.5
    ret, calls, T, flags, idx = _run_adapter(poseopt_main, tmp_path, s, has_mp, preset)
    assert calls == 1 and ret == ref.n_good
    assert np.array_equal(flags[~has_mp], preset[~has_mp]) and np.array_equal(flags[idx], ref.outlier)
    scale = max(1.0, float(np.abs(ref.Tcw).max()))
    assert np.abs(T.astype(np.float64) - ref.Tcw).max() <= 2 * ULP * scale
    s2 = scene(**size_scene(2))
    has2 = np.zeros(6, bool)
    has2[[1, 4]] = True
    ret, calls, T, flags, idx = _run_adapter(poseopt_main, tmp_path, s2, has2, np.ones(6, bool))
    assert (ret, calls) == (0, 0) and flags.tolist() == [True, False, True, True, False, True]
    assert T[:3].tobytes() == s2["Tcw0"][:3].tobytes()
