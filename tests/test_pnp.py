"""PnPsolver row: EPnP + RANSAC on the GPU against the
numpy oracle (oracle/pnp_ref.py).

Tolerance (floating point, the north star's "PnP pose within a stated float
tolerance"): the refined pose Tcw of the GPU and of the oracle agree to
|dR|_max <= 1e-3 and |dt|_max <= 1e-3 * (1 + |t|_max); integer outcomes
(found, iterations consumed, best inlier count) must be identical, and the
inlier masks may differ in at most 1 % of the correspondences (points whose
reprojection error sits on the 5.991 sigma^2 threshold).  The best
hypothesis' pose and mask are held to the same tolerance, a mask's sum equals
its count exactly, and a pose the call did not produce is all zeros
(_check_record).  The problems come from tests/pnp_cases.py."""
import ctypes
import math
from functools import lru_cache

import numpy as np
import pytest

import pnp_cases
import pnp_ref
import synth

LIBC = ctypes.CDLL("libc.so.6")


def _ransac():
    import ransac
    return ransac


def test_qr_solve_restatement_is_least_squares():
    rng = np.random.default_rng(0)
    for _ in range(20):
        A = rng.normal(size=(6, 4))
        b = rng.normal(size=6)
        np.testing.assert_allclose(pnp_ref._qr_solve(A, b), np.linalg.lstsq(A, b, rcond=None)[0], atol=1e-9)


def _qr_cases():
    """6 x 4 systems whose LAST row holds a column's largest magnitude: the
    reference's eta scan (PnPsolver.cpp:975-980) never reads the last row, so
    eta -- and the rounding of every later step -- differs from a scan over
    all rows; plus a system the reference calls singular (rows k .. nr-2 of
    column 0 zero, the last row not): it returns with X untouched."""
    rng = np.random.default_rng(7)
    cases = []
    for t in range(32):
        A = rng.normal(size=(6, 4))
        A[5, t % 4] = 40.0 * (1 + rng.random())  # last row: the column maximum
        cases.append((A, rng.normal(size=6)))
    A = rng.normal(size=(6, 4))
    A[:5, 0] = 0.0
    cases.append((A, rng.normal(size=6)))
    return cases


def _qr_all_rows(A, b):
    """the same Householder QR with eta over ALL rows and a division (the
    pre-round-4 restatement): what the letter-faithful scan must differ from"""
    A = A.copy()
    b = b.copy()
    nr, nc = A.shape
    A1, A2 = np.zeros(nc), np.zeros(nc)
    for k in range(nc):
        eta = np.abs(A[k:, k]).max()
        A[k:, k] /= eta
        sigma = np.sqrt((A[k:, k] ** 2).sum())
        sigma = -sigma if A[k, k] < 0 else sigma
        A[k, k] += sigma
        A1[k], A2[k] = sigma * A[k, k], -eta * sigma
        for j in range(k + 1, nc):
            tau = (A[k:, k] * A[k:, j]).sum() / A1[k]
            A[k:, j] -= tau * A[k:, k]
    for j in range(nc):
        b[j:] -= (A[j:, j] * b[j:]).sum() / A1[j] * A[j:, j]
    X = np.zeros(nc)
    X[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        X[i] = (b[i] - (A[i, i + 1:] * X[i + 1:]).sum()) / A2[i]
    return X


def _qr_cpp(A, b, X0):
    import ctypes
    import orbref
    L = orbref.lib()
    f = L.orbref_qr_solve_6x4
    f.argtypes = [ctypes.c_void_p] * 3
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    X = np.array(X0, np.float64)
    f(A.ctypes.data, b.ctypes.data, X.ctypes.data)
    return X


def test_qr_solve_eta_scan_is_the_references():
    """oracle/pnp_ref.py == oracle/pnp_ref.cpp bit for bit on the eta-scan
    cases; the last-row-maximum systems differ in rounding from an all-rows
    scan on some systems (the scan is observable), and the singular case
    leaves X as it was."""
    cases = _qr_cases()
    X0 = np.array([0.25, -1.5, 3.0, 7.0])
    differ = 0
    for A, b in cases[:-1]:
        xp = pnp_ref._qr_solve(A, b, X0)
        xc = _qr_cpp(A, b, X0)
        assert xp.tobytes() == xc.tobytes()
        np.testing.assert_allclose(xp, np.linalg.lstsq(A, b, rcond=None)[0], rtol=1e-9, atol=1e-9)
        differ += xp.tobytes() != _qr_all_rows(A, b).tobytes()
    assert differ > 0
    A, b = cases[-1]
    assert pnp_ref._qr_solve(A, b, X0).tobytes() == X0.tobytes()
    assert _qr_cpp(A, b, X0).tobytes() == X0.tobytes()


@pytest.mark.gpu
def test_gpu_qr_solve_eta_scan_equals_oracle():
    """csrc/epnp.h qr_solve_6x4 (the EPnP Gauss-Newton solve on the GPU) on
    the same cases, through orbgpu_debug_qr_solve_6x4_device: bit-identical
    to the oracle, the singular case leaving X untouched"""
    import ctypes
    import orbgpu
    import torch
    cases = _qr_cases()
    X0 = np.array([0.25, -1.5, 3.0, 7.0])
    A = torch.tensor(np.stack([a.reshape(-1) for a, _ in cases]), dtype=torch.float64, device="cuda")
    b = torch.tensor(np.stack([bb for _, bb in cases]), dtype=torch.float64, device="cuda")
    X = torch.tensor(np.tile(X0, (len(cases), 1)), dtype=torch.float64, device="cuda")
    f = orbgpu.lib().orbgpu_debug_qr_solve_6x4_device
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    assert f(A.data_ptr(), b.data_ptr(), X.data_ptr(), len(cases), None) == 0
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    for i, (a, bb) in enumerate(cases):
        assert got[i].tobytes() == pnp_ref._qr_solve(a, bb, X0).tobytes(), i


def test_epnp_minimal_sets_mostly_accurate():
    """EPnP on 4 noise-free points is approximate (three beta linearisations +
    5 Gauss-Newton steps); with the canonical null-space basis most minimal
    sets land within a few pixels, as RANSAC needs."""
    errs = []
    for trial in range(100):
        P = synth.pnp_problem(4, 1.0, seed=500 + trial, noise_px=0.0)
        errs.append(pnp_ref.compute_pose(P["P3w"].astype(np.float64), P["P2"].astype(np.float64), P["cam"])[2])
    assert np.mean(np.array(errs) < 5.0) >= 0.6


@pytest.mark.parametrize("n", [6, 50])
def test_epnp_oracle_exact_on_noise_free_points(n):
    P = synth.pnp_problem(n, 1.0, seed=n, noise_px=0.0)
    R, t, err = pnp_ref.compute_pose(P["P3w"].astype(np.float64), P["P2"].astype(np.float64), P["cam"])
    assert err < 1e-3
    np.testing.assert_allclose(R, P["R"], atol=1e-5)
    np.testing.assert_allclose(t, P["t"], atol=1e-4)


def test_set_ransac_parameters_like_tracking():
    """SetRansacParameters(0.99,10,300,4,0.5,5.991) (Tracking.cpp:1796; PnPsolver.cpp:159-195)."""
    ransac = _ransac()
    for n, expect_min in [(30, 15), (15, 10), (9, 10), (201, 100)]:
        P = synth.pnp_problem(n, 0.5, seed=1)
        s = ransac.PnPsolver(P["P3w"], P["P2"], P["sigma2"], *P["cam"])
        s.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
        assert s.min_inliers == max(int(np.float32(n) * np.float32(0.5)), 10, 4) == expect_min
        eps = max(np.float32(0.5), np.float32(s.min_inliers) / np.float32(n))
        if s.min_inliers == n:
            assert s.max_its == 1
        elif eps < 1:
            assert s.max_its == max(1, min(300, math.ceil(math.log(0.01) / math.log(1 - float(eps) ** 3))))
        np.testing.assert_array_equal(s.maxerr, P["sigma2"] * np.float32(5.991))


def test_oracle_ransac_finds_pose():
    P = synth.pnp_problem(120, 0.5, seed=7)
    rng = np.random.default_rng(3)
    samples = np.stack([rng.choice(120, 4, replace=False) for _ in range(300)])
    maxerr = P["sigma2"] * np.float32(5.991)
    r = pnp_ref.ransac_call(P["P3w"], P["P2"], maxerr, P["cam"], 40, 0, np.zeros(120, bool), samples)
    assert r["found"] == 1
    np.testing.assert_allclose(r["refined_R"], P["R"], atol=5e-3)
    assert (r["refined_mask"] & P["inlier"]).sum() >= 0.95 * P["inlier"].sum()


def _pose_close(Tg, R, t):
    Tg = np.asarray(Tg, np.float64).reshape(4, 4)
    assert np.abs(Tg[:3, :3] - R).max() <= 1e-3
    assert np.abs(Tg[:3, 3] - t).max() <= 1e-3 * (1 + np.abs(t).max())


def _oracle_cases():
    rng = np.random.default_rng(9)
    cases = []
    for b in range(16):
        n = int(rng.integers(12, 300))
        frac = [0.0, 0.3, 0.5, 0.8, 1.0][b % 5]
        P = synth.pnp_problem(n, frac, seed=200 + b)
        n_hyp = int(rng.integers(1, 200))
        samples = np.stack([rng.choice(n, 4, replace=False) for _ in range(n_hyp)]).astype(np.int32)
        min_inl = max(int(np.float32(n) * np.float32(0.5)), 10)
        cases.append((P, samples, min_inl))
    return cases


def _run_batch(cases, refined_fill=0):
    """(P, samples, min_inliers[, best_inliers, best_mask]) cases as one orbgpu_pnp_ransac_batch call
    (the last two: the state carried into the call, 0 and an all-zero mask when left out): the
    problem records, the result records and the best and refined masks.  The refined mask goes in
    holding refined_fill in every byte."""
    ransac = _ransac()
    arr = (ransac.PnPProblem * len(cases))()
    P3, P2, E, S, BM = [], [], [], [], []
    off = soff = 0
    for b, case in enumerate(cases):
        P, samples, min_inl = case[:3]
        p = arr[b]
        n = len(P["P3w"])
        best, mask = (case[3], case[4]) if len(case) > 3 else (0, np.zeros(n, np.uint8))
        assert len(mask) == n
        p.n, p.offset, p.min_inliers, p.best_inliers, p.n_hyp, p.sample_offset = n, off, min_inl, best, len(samples), soff
        p.fu, p.fv, p.uc, p.vc = P["cam"]
        P3.append(P["P3w"]); P2.append(P["P2"]); E.append(P["sigma2"] * np.float32(5.991))
        S.append(np.asarray(samples, np.int32).reshape(-1, 4)); BM.append(np.asarray(mask, np.uint8))
        off += n; soff += len(samples)
    bm = np.concatenate(BM)
    rm = np.full(off, refined_fill, np.uint8)
    res = ransac.pnp_ransac_batch(arr, np.concatenate(P3), np.concatenate(P2), np.concatenate(E),
                                  np.concatenate(S), bm, rm)
    return arr, res, bm, rm


ZERO_POSE = bytes(64)  # the empty cv::Mat of a pose the call did not produce


def _slices(arr, b, *masks):
    off, n = arr[b].offset, arr[b].n
    return [m[off:off + n] for m in masks]


def _check_record(g, o, case, bm, rm, label):
    """every word of the result record g and both masks of one problem against the oracle's o at
    the file's tolerance: integers equal, poses within _pose_close, masks within the cap; a mask's
    sum equal to its count exactly (both come from the same pnp_inlier on the same double pose);
    a pose the call did not produce all zeros, and the best mask then as it came in"""
    n = len(case[0]["P3w"])
    cap = max(1, n // 100)
    assert (g.found, g.consumed, g.best_hyp, g.best_inliers) == pnp_cases.outcome(o), label
    if g.best_hyp >= 0:
        _pose_close(g.best_Tcw, o["best_R"], o["best_t"])
        diff = int((bm.astype(bool) != o["best_mask"]).sum())
        assert diff <= cap, f"{label}: {diff} best-mask differences"
        assert int(bm.sum()) == g.best_inliers, label
    else:
        assert bytes(g.best_Tcw) == ZERO_POSE, label
        incoming = np.asarray(case[4], np.uint8) if len(case) > 3 else np.zeros(n, np.uint8)
        assert bm.tobytes() == incoming.tobytes(), label
    if g.found:
        _pose_close(g.refined_Tcw, o["refined_R"], o["refined_t"])
        diff = int((rm.astype(bool) != o["refined_mask"]).sum())
        assert diff <= cap, f"{label}: {diff} refined-mask differences"
        assert abs(g.refined_inliers - int(o["refined_mask"].sum())) <= cap, label
        assert int(rm.sum()) == g.refined_inliers, label
    else:
        assert bytes(g.refined_Tcw) == ZERO_POSE, label
        assert g.refined_inliers == 0, label


def _check_batch(cases, oracles, run=None):
    arr, res, bm, rm = run or _run_batch(cases)
    for b, (case, o) in enumerate(zip(cases, oracles)):
        _check_record(res[b], o, case, *_slices(arr, b, bm, rm), f"case {b}")
    return arr, res, bm, rm


@pytest.mark.gpu
def test_pnp_gpu_batch_vs_oracle():
    cases = _oracle_cases()
    arr, res, bm, rm = _run_batch(cases)
    nfound = 0
    for b, (P, samples, min_inl) in enumerate(cases):
        g = res[b]
        n = len(P["P3w"])
        o = pnp_ref.ransac_call(P["P3w"], P["P2"], P["sigma2"] * np.float32(5.991), P["cam"], min_inl, 0,
                                np.zeros(n, bool), samples)
        assert (g.found, g.consumed, g.best_inliers) == (o["found"], o["consumed"], o["best_inliers"]), f"case {b}"
        off_b = arr[b].offset
        if o["found"]:
            nfound += 1
            _pose_close(g.refined_Tcw, o["refined_R"], o["refined_t"])
            diff = (rm[off_b:off_b + n].astype(bool) != o["refined_mask"]).sum()
            assert diff <= max(1, n // 100), f"case {b}: {diff} refined-mask differences"
            assert abs(g.refined_inliers - int(o["refined_mask"].sum())) <= max(1, n // 100)
        _check_record(g, o, cases[b], *_slices(arr, b, bm, rm), f"case {b}")
    assert nfound >= 6


@pytest.mark.gpu
def test_pnp_solver_iterate_consumes_the_reference_stream():
    """PnPsolver.iterate(5) like Tracking::Relocalization (Tracking.cpp:1815-1830):
    outcome and random-stream position equal a sequential replay with the
    oracle drawing from glibc itself."""
    ransac = _ransac()
    P = synth.pnp_problem(80, 0.6, seed=77)
    ransac.srand(0)
    s = ransac.PnPsolver(P["P3w"], P["P2"], P["sigma2"], *P["cam"])
    s.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, no_more, inl, n = s.iterate(5)
    # replay: the `||` loop runs max(maxIts - 0, 5) iterations unless Refine succeeds
    LIBC.srand(0)
    N = len(P["P3w"])
    samples = []
    for _ in range(max(s.max_its, 5)):
        avail = list(range(N))
        tri = []
        for _ in range(4):
            r = int((LIBC.rand() / (2147483647 + 1.0)) * len(avail))
            tri.append(avail[r]); avail[r] = avail[-1]; avail.pop()
        samples.append(tri)
    o = pnp_ref.ransac_call(P["P3w"], P["P2"], s.maxerr, P["cam"], s.min_inliers, 0, np.zeros(N, bool),
                            np.array(samples))
    assert o["found"] == 1 and T is not None
    assert s.iterations == o["consumed"]
    _pose_close(T, o["refined_R"], o["refined_t"])
    # rewind glibc to the position the reference would be at
    LIBC.srand(0)
    for _ in range(4 * o["consumed"]):
        LIBC.rand()
    assert [ransac.rand() for _ in range(5)] == [LIBC.rand() for _ in range(5)]


# --------------------------------------------------------------------------
# every output word and code path of orbgpu_pnp_ransac_batch (tests/pnp_cases.py)
# --------------------------------------------------------------------------
def test_pnp_cases_held_best_and_carried_state_in_the_oracle():
    """what the GPU tests of the held best, the padded replay and the carried state lean on"""
    for k in pnp_cases.HELD_K:
        case = pnp_cases.held_best_case(k)
        assert len(case[1]) == pnp_cases.HELD_OUTCOME[k][1]
        assert pnp_cases.outcome(pnp_cases.oracle(case)) == pnp_cases.HELD_OUTCOME[k], k
    whole = pnp_cases.padded_oracle()
    assert pnp_cases.outcome(whole) == pnp_cases.PADDED_OUTCOME
    o1, o2, o3 = pnp_cases.carried_oracles()
    assert tuple(pnp_cases.outcome(o) for o in (o1, o2, o3)) == pnp_cases.CARRIED_OUTCOME
    assert o1["best_mask"].tobytes() == o2["best_mask"].tobytes() == whole["best_mask"].tobytes()
    assert o3["refined_inliers"] == 6 and o3["best_mask"].tobytes() == o1["best_mask"].tobytes()


def test_pnp_cases_chunk_boundary_in_the_oracle():
    for key in pnp_cases.CHUNK:
        o = pnp_cases.chunk_oracle(*key)
        assert pnp_cases.outcome(o)[:3] == pnp_cases.CHUNK_OUTCOME[key], key


def test_pnp_cases_refine_sets_exact_in_the_oracle():
    """Refine on m chosen noise-free points: the oracle finds the true pose (the bounds of
    test_epnp_oracle_exact_on_noise_free_points; measured 1.5e-7 on R and 1.1e-6 on t at most)"""
    for m in pnp_cases.REFINE_M:
        case = pnp_cases.refine_set_case(m)
        o = pnp_cases.oracle(case)
        assert pnp_cases.outcome(o) == (1, 1, -1, 320) and o["refined_inliers"] == 320, m
        np.testing.assert_allclose(o["refined_R"], case[0]["R"], atol=1e-5)
        np.testing.assert_allclose(o["refined_t"], case[0]["t"], atol=1e-4)


def test_pnp_cases_single_hypotheses_and_eigen_path_in_the_oracle():
    _, _, counts = pnp_cases.single_hyp_sets()
    assert int((counts >= 4).sum()) == 49
    assert int(((counts == 3) | (counts == 4)).sum()) <= 2 and int((counts > 4).sum()) >= 32
    for case in pnp_cases.eigen_path_cases():
        X = case[1][0]
        assert len(set(X.tolist())) == 4 and X.min() >= 6
        assert pnp_cases.outcome(pnp_cases.oracle(case))[:3] == (1, 1, 0)
    D = pnp_cases.eigen_path_cases()[0][1][1:]
    P3 = pnp_cases.eigen_path_cases()[0][0]["P3w"]
    assert all(len(np.unique(P3[d], axis=0)) < 4 for d in D)  # each holds a 3D point twice


@pytest.mark.gpu
@pytest.mark.parametrize("k", pnp_cases.HELD_K)
def test_pnp_gpu_best_held_without_refined_pose(k):
    """RANSAC runs out holding hypothesis 0 as its best and Refine never succeeds: the record that
    PnPsolver::iterate serves mBestTcw and mvbBestInliers from (PnPsolver.cpp:284-297); Refine's
    EPnP ran on k = 4, 5, 6, 10 correspondences"""
    case = pnp_cases.held_best_case(k)
    _check_batch([case], [pnp_cases.oracle(case)])


@pytest.mark.gpu
def test_pnp_gpu_best_held_across_the_chunk_boundary():
    """300 hypotheses: the best of hypothesis 0 is held over both LDS chunks of the replay"""
    _check_batch([pnp_cases.padded_case()], [pnp_cases.padded_oracle()])


@lru_cache(maxsize=None)
def _chunk_batch():
    cases = [pnp_cases.chunk_case(*key) for key in pnp_cases.CHUNK]
    return (cases,) + tuple(_run_batch(cases))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(pnp_cases.CHUNK)))
def test_pnp_gpu_first_qualifying_hypothesis_around_the_chunk_boundary(i):
    """the first hypothesis that qualifies is number 255 .. 299 of 300, on either side of the replay's
    chunk of 256 (or none qualifies and Refine fails): one batch of five, a case per parameter"""
    cases, arr, res, bm, rm = _chunk_batch()
    o = pnp_cases.chunk_oracle(*pnp_cases.CHUNK[i])
    assert pnp_cases.outcome(o)[:3] == pnp_cases.CHUNK_OUTCOME[pnp_cases.CHUNK[i]]
    _check_record(res[i], o, cases[i], *_slices(arr, i, bm, rm), f"case {pnp_cases.CHUNK[i]}")


@pytest.mark.gpu
def test_pnp_gpu_chunk_boundary_problem_alone():
    case = pnp_cases.chunk_case(42, 256)
    _check_batch([case], [pnp_cases.chunk_oracle(42, 256)])


@pytest.mark.gpu
def test_pnp_gpu_carried_state():
    """the in/out contract of best_inliers and best_mask, as a second iterate() on one solver uses
    it: call 2 gets call 1's count and its downloaded mask; with min_inliers = 5 its first
    hypothesis runs Refine on the carried mask"""
    o1, o2, o3 = pnp_cases.carried_oracles()
    c1 = pnp_cases.carried_cases(0, None)[0]
    arr, res, bm, rm = _check_batch([c1, pnp_cases.padded_case()], [o1, pnp_cases.padded_oracle()])
    bm1, bm_whole = _slices(arr, 0, bm)[0].copy(), _slices(arr, 1, bm)[0]
    _, c2, c3 = pnp_cases.carried_cases(res[0].best_inliers, bm1)
    arr, res, bm, rm = _check_batch([c2, c3], [o2, o3])
    for b in range(2):  # the carried mask is left as it came in, and is the single 300-hypothesis run's
        assert _slices(arr, b, bm)[0].tobytes() == bm1.tobytes() == bm_whole.tobytes()
    assert res[1].refined_inliers == 6


@pytest.mark.gpu
def test_pnp_gpu_no_work_members_of_a_batch():
    """n_hyp = 0 with carried state, and n = 0, beside a working problem: nothing consumed, the count
    passed through, both masks as they came in, zero poses"""
    P, samples, min_inl = pnp_cases.held_best_case(6)
    carried = np.zeros(30, np.uint8)
    carried[[0, 2, 3, 7, 11, 29]] = 1
    none = np.zeros((0, 4), np.int32)
    empty = {"P3w": np.zeros((0, 3), np.float32), "P2": np.zeros((0, 2), np.float32),
             "sigma2": np.zeros(0, np.float32), "cam": P["cam"]}
    cases = [(P, none, min_inl, 6, carried), (P, samples, min_inl), (empty, none, 4, 3, np.zeros(0, np.uint8)),
             (P, none, min_inl, 6, carried)]
    oracles = [pnp_cases.oracle(c) for c in cases]
    arr, res, bm, rm = _check_batch(cases, oracles, run=_run_batch(cases, refined_fill=7))
    for b in (0, 2, 3):
        g = res[b]
        assert (g.found, g.consumed, g.best_hyp, g.best_inliers, g.refined_inliers) == (0, 0, -1, cases[b][3], 0)
        assert bytes(g.best_Tcw) == bytes(g.refined_Tcw) == ZERO_POSE
        m_best, m_ref = _slices(arr, b, bm, rm)
        assert m_best.tobytes() == cases[b][4].tobytes() and (m_ref == 7).all()


@pytest.mark.gpu
def test_pnp_gpu_refine_on_chosen_sets_vs_truth():
    """Refine's wave-wide EPnP on exactly m = 4 .. 320 chosen noise-free points (k = 4, 2, 0 null
    vectors to canonicalise; m on either side of its lane strides 16 and 64 and of 256), one batch
    of 18: against the oracle at the file tolerance, and against the true pose -- independent of
    both restatements -- at the bounds the oracle itself meets"""
    cases = [pnp_cases.refine_set_case(m) for m in pnp_cases.REFINE_M]
    oracles = [pnp_cases.oracle(c) for c in cases]
    arr, res, bm, rm = _check_batch(cases, oracles)
    worst_R = worst_t = 0.0
    for m, case, g in zip(pnp_cases.REFINE_M, cases, res):
        assert (g.found, g.consumed, g.best_hyp, g.best_inliers, g.refined_inliers) == (1, 1, -1, 320, 320), m
        T = np.array(g.refined_Tcw, np.float64).reshape(4, 4)
        dR, dt = np.abs(T[:3, :3] - case[0]["R"]).max(), np.abs(T[:3, 3] - case[0]["t"]).max()
        print(f"m = {m}: |dR| = {dR:.3g}, |dt| = {dt:.3g} against the truth")
        worst_R, worst_t = max(worst_R, dR), max(worst_t, dt)
        np.testing.assert_allclose(T[:3, :3], case[0]["R"], rtol=0, atol=1e-5, err_msg=f"m = {m}")
        np.testing.assert_allclose(T[:3, 3], case[0]["t"], rtol=0, atol=1e-4, err_msg=f"m = {m}")
    print(f"worst against the truth: |dR| = {worst_R:.3g}, |dt| = {worst_t:.3g}")


@pytest.mark.gpu
def test_pnp_gpu_every_minimal_set_one_per_problem():
    """64 minimal sets, each the only hypothesis of a problem of its own with min_inliers = 4, so
    every set's pose, count and mask surface as the best (in a RANSAC run half the hypotheses score 0
    and are never seen).  Sets whose oracle count is 3 or 4 sit on the threshold and are dropped."""
    P, sets, counts = pnp_cases.single_hyp_sets()
    cases = [(P, s[None], 4) for s in sets]
    arr, res, bm, rm = _run_batch(cases)
    pw, us = P["P3w"].astype(np.float64), P["P2"].astype(np.float64)
    cam = tuple(float(c) for c in P["cam"])
    cap = max(1, 60 // 100)
    kept = 0
    for b, (s, c) in enumerate(zip(sets, counts)):
        if c in (3, 4):
            continue
        g = res[b]
        if c < 4:
            assert g.best_hyp == -1 and g.best_inliers == 0 and bytes(g.best_Tcw) == ZERO_POSE, b
            continue
        kept += 1
        R, t, _ = pnp_ref.compute_pose(pw[s], us[s], cam)
        mask = pnp_ref.check_inliers(R, t, P["P3w"], P["P2"], pnp_cases.maxerr(P), cam)
        m_best = _slices(arr, b, bm)[0]
        assert g.best_hyp == 0 and abs(g.best_inliers - c) <= cap, (b, g.best_inliers, c)
        assert int((m_best.astype(bool) != mask).sum()) <= cap and int(m_best.sum()) == g.best_inliers, b
        _pose_close(g.best_Tcw, R, t)
    assert kept >= 32 and int(np.isin(counts, (3, 4)).sum()) <= 2


@pytest.mark.gpu
def test_pnp_gpu_regular_set_on_the_eigen_path():
    """a regular minimal set whose wave neighbours are degenerate takes null_space_from_mtm<16>
    instead of the 12 x 12 solve: same best pose and mask as beside regular neighbours, and as the
    oracle's.  Nothing is asserted on the degenerate sets themselves."""
    cases = list(pnp_cases.eigen_path_cases())
    oracles = [pnp_cases.oracle(c) for c in cases]
    arr, res, bm, rm = _check_batch(cases, oracles)
    assert all((g.found, g.consumed, g.best_hyp) == (1, 1, 0) for g in res)
    Ta, Tb = (np.array(g.best_Tcw, np.float64).reshape(4, 4) for g in res)
    _pose_close(Ta, Tb[:3, :3], Tb[:3, 3])
    (ma,), (mb,) = _slices(arr, 0, bm), _slices(arr, 1, bm)
    assert int((ma != mb).sum()) <= max(1, 60 // 100)


@pytest.mark.gpu
def test_pnp_gpu_batch_equals_alone():
    """every byte of each result record and of both masks is the same from a batch as from the
    problem run alone (all bytes of the record are defined)"""
    for cases, run in ((pnp_cases.six_cases(), None), (_chunk_batch()[0], _chunk_batch()[1:])):
        arr, res, bm, rm = run or _run_batch(cases)
        for b, case in enumerate(cases):
            arr1, res1, bm1, rm1 = _run_batch([case])
            assert bytes(res[b]) == bytes(res1[0]), b
            m_best, m_ref = _slices(arr, b, bm, rm)
            assert m_best.tobytes() == bm1.tobytes() and m_ref.tobytes() == rm1.tobytes(), b
