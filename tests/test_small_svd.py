"""csrc/small_svd.h (sym_eig_desc, svd_hestenes, svd_solve) and csrc/epnp.h's qr_solve_6x4, compiled
for the host (tests/cpp/small_svd_main.cpp, with the library's -ffp-contract=off and under the host
sanitizers): what EPnP's kernels take from them, stated where a CPU can check it."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pnp_ref
import test_pnp

ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
# of eps sigma_max.  A numerically null column (squared norm below kJacobiNegl = 1e-28 of ||A||_F^2)
# takes no further rotation, so a rank-deficient matrix may keep up to 1e-14 ||A||_F = 45 eps ||A||_F
# where numpy has ~0: the singular values of the matrices below reach 32 units, the other figures 8.
UNITS = 64


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    subprocess.run(["make", "-C", str(ROOT / "tests" / "cpp"), "small_svd_main"], check=True, capture_output=True)
    exe = ROOT / "tests" / "cpp" / "small_svd_main"
    tmp = tmp_path_factory.mktemp("small_svd")

    def run(mode, records, width_out):
        src, dst = tmp / f"{mode}_in.bin", tmp / f"{mode}_out.bin"
        np.ascontiguousarray(records, np.float64).tofile(src)
        r = subprocess.run([str(exe), mode, str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr  # the sanitizers report on stderr and fail the run
        return np.fromfile(dst, np.float64).reshape(len(records), width_out)

    return run


def test_qr_solve_6x4_equals_the_oracle_byte_for_byte(run):
    cases = test_pnp._qr_cases()
    assert len(cases) == 33
    X0 = np.array([0.25, -1.5, 3.0, 7.0])
    got = run("qr", [np.concatenate([A.reshape(-1), b, X0]) for A, b in cases], 4)
    for i, (A, b) in enumerate(cases):
        assert got[i].tobytes() == pnp_ref._qr_solve(A, b, X0).tobytes(), i
    assert got[-1].tobytes() == X0.tobytes()  # the singular system leaves X as it was


def test_zero_columns_leave_the_smaller_systems_solution(run):
    """The beta approximations' 6 x 4 and 6 x 3 systems are solved as 6 x 5 with zero columns
    (epnp.h, solve_beta_approximation): the result is the smaller system's byte for byte and the
    padded unknowns are exactly 0."""
    rng = np.random.default_rng(23)
    records = []
    for i in range(300):
        scale = 10.0 ** rng.uniform(-3, 3)
        L = rng.normal(size=(6, 10)) * scale
        if i % 5 == 0:
            L[:, 1] = 2.0 * L[:, 0]
        records.append(np.concatenate([L.reshape(-1), rng.normal(size=6) * scale]))
    got = run("zero", records, 17)
    wide1, small1, wide2, small2 = got[:, :5], got[:, 5:9], got[:, 9:14], got[:, 14:17]
    assert np.isfinite(got).all()
    assert wide1[:, :4].tobytes() == small1.tobytes()
    assert wide2[:, :3].tobytes() == small2.tobytes()
    assert wide1[:, 4:].tobytes() == np.zeros((300, 1)).tobytes()
    assert wide2[:, 3:].tobytes() == np.zeros((300, 2)).tobytes()
    assert np.abs(small1).max() > 0 and np.abs(small2).max() > 0


def _matrices(n, count=300):
    """seeded n x n matrices over scales 1e-3 .. 1e3, every fifth rank-deficient, every seventh
    (n = 4) with a zero fourth column"""
    rng = np.random.default_rng(11)
    out = []
    for i in range(count):
        A = rng.normal(size=(n, n)) * 10.0 ** rng.uniform(-3, 3)
        if i % 5 == 0:
            A[:, 1] = A[:, 0] - 0.5 * A[:, 2]
        if i % 7 == 0 and n == 4:
            A[:, 3] = 0.0
        out.append(A)
    return out


@pytest.mark.parametrize("n", [3, 4])
def test_svd_hestenes_against_numpy(run, n):
    mats = _matrices(n)
    got = run(f"svd{n}", [A.reshape(-1) for A in mats], n + 2 * n * n)
    worst = np.zeros(3)
    for A, rec in zip(mats, got):
        s, V, Us = rec[:n], rec[n:n + n * n].reshape(n, n), rec[n + n * n:].reshape(n, n)
        want = np.linalg.svd(A, compute_uv=False)
        unit = EPS * want[0]
        worst = np.maximum(worst, [np.abs(np.sort(s)[::-1] - want).max() / unit,
                                   np.abs(V.T @ V - np.eye(n)).max() / EPS,
                                   np.abs(Us @ V.T - A).max() / unit])
    print(f"svd_hestenes<{n},{n}>: singular values, V^T V - I, (U s) V^T - A in units of eps sigma_max:", worst)
    assert (worst <= UNITS).all(), worst


def test_sym_eig_desc_against_numpy(run):
    mats = [A.T @ A for A in _matrices(3)]
    got = run("eig3", [S.reshape(-1) for S in mats], 12)
    worst = 0.0
    for S, rec in zip(mats, got):
        want = np.linalg.eigvalsh(S)[::-1]
        assert (np.diff(rec[:3]) <= 0).all()  # descending
        worst = max(worst, np.abs(rec[:3] - want).max() / (EPS * np.linalg.svd(S, compute_uv=False)[0]))
    print("sym_eig_desc<3>: eigenvalues in units of eps sigma_max:", worst)
    assert worst <= UNITS, worst
