"""csrc/lm_device.h's Cholesky solve, compiled for the host (tests/cpp/lm_solve_main.cpp, with
the library's -ffp-contract=off and under the host sanitizers), against tests/lm_ref.py byte for
byte: the two kernels and the two restatements solve with these two functions."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lm_ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lm_solve_main():
    subprocess.run(["make", "-C", str(ROOT / "tests" / "cpp"), "lm_solve_main"], check=True, capture_output=True)
    return ROOT / "tests" / "cpp" / "lm_solve_main"


def _third_pivot_terms(H):
    """what the first two columns of L take from H[2][2], in the solve's operations"""
    l00 = np.sqrt(H[0, 0])
    l10, l20 = H[0, 1] / l00, H[0, 2] / l00
    l11 = np.sqrt(H[1, 1] - l10 * l10)
    l21 = (H[1, 2] - l20 * l10) / l11
    return l20 * l20, l21 * l21


@functools.lru_cache(maxsize=None)
def _system_cached(n):
    """H = J^T J + I of a seeded J (20 x n), b, lambda.  The seed is the first from 900 whose
    a + c below is a double, so that one diagonal entry can make the third pivot exactly zero
    (h - a and then - c are exact differences: with any other h the pivot is a rounding error)."""
    for seed in range(900, 1900):
        rng = np.random.default_rng(seed)
        J = rng.normal(size=(20, n))
        H = J.T @ J + np.eye(n)
        a, c = _third_pivot_terms(H)
        if ((a + c) - a) - c == 0.0:
            return H, rng.normal(size=n), 0.37
    raise AssertionError("no seed")


def _system(n):
    H, b, lam = _system_cached(n)
    return H.copy(), b.copy(), lam


def _zero_third_pivot(n):
    """the same H with H[2][2] = L20^2 + L21^2 and lambda = 0: the third pivot is exactly zero"""
    H, b, _ = _system(n)
    a, c = _third_pivot_terms(H)
    H[2, 2] = a + c
    return H, b, 0.0


def _with_nan(n):
    H, b, lam = _system(n)
    H[1, 3] = H[3, 1] = np.nan
    return H, b, lam


@pytest.mark.parametrize("n", [6, 7])
@pytest.mark.parametrize("case,solvable", [(_system, True), (_zero_third_pivot, False), (_with_nan, False)],
                         ids=["well_conditioned", "zero_third_pivot", "nan_in_H"])
def test_host_solve_equals_the_restatement_byte_for_byte(lm_solve_main, tmp_path, n, case, solvable):
    H, b, lam = case(n)
    x = lm_ref.cholesky_solve(H, b, lam)
    assert (x is not None) == solvable
    upper = [H[j, k] for j in range(n) for k in range(j, n)]
    np.array([n, *upper, *b, lam], np.float64).tofile(tmp_path / "in.bin")
    r = subprocess.run([str(lm_solve_main), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # the sanitizers report on stderr and fail the run
    want = np.array([1.0, *x] if solvable else [0.0], np.float64)
    assert (tmp_path / "out.bin").read_bytes() == want.tobytes()
    if solvable:
        A = H + lam * np.eye(n)
        assert np.abs(A @ np.array(x) - b).max() <= 1e-12 * np.abs(A).max() * max(1.0, np.abs(x).max()) * n
