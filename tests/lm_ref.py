"""What the CPU restatements of the two dense optimisers share (poseopt_ref.py,
sim3opt_ref.py), as csrc/lm_device.h does for the kernels: g2o's
OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.
cpp:61-189) on one free vertex, the Cholesky solve of (H + lam I) x = b whose
non-positive pivot is the failed solve, Huber's robustify and Eigen 3's
quaternion algebra as recalled (Quaternion(Matrix3), operator*,
_transformVector, toRotationMatrix).
Sequential float64 in Python float arithmetic, one IEEE operation per
expression node, written in the kernels' association order.
"""
import math
from types import SimpleNamespace

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return float("nan") if a == 0 or a != a else math.copysign(float("inf"), a) * math.copysign(1.0, b)


# ---------------------------------------------------------------- quaternions: q = (x, y, z, w)

def quat_from_R(R):
    """Eigen: Quaterniond(Matrix3d)"""
    t = (R[0][0] + R[1][1]) + R[2][2]
    q = [0.0] * 4
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2][1] - R[1][2]) * t
        q[1] = (R[0][2] - R[2][0]) * t
        q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = ((R[i][i] - R[j][j]) - R[k][k]) + 1.0
        t = math.sqrt(s) if s >= 0 else float("nan")
        q[i] = 0.5 * t
        t = 0.5 / t if t != 0 else float("inf")
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    return q


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [((aw * bx + ax * bw) + ay * bz) - az * by,
            ((aw * by + ay * bw) + az * bx) - ax * bz,
            ((aw * bz + az * bw) + ax * by) - ay * bx,
            ((aw * bw - ax * bx) - ay * by) - az * bz]


def quat_rotate(q, v):
    """Eigen's _transformVector on v = (x, y, z) scalars or arrays"""
    qx, qy, qz, qw = q
    ux = qy * v[2] - qz * v[1]
    uy = qz * v[0] - qx * v[2]
    uz = qx * v[1] - qy * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return ((v[0] + qw * ux) + (qy * uz - qz * uy),
            (v[1] + qw * uy) + (qz * ux - qx * uz),
            (v[2] + qw * uz) + (qx * uy - qy * ux))


def quat_to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


# ---------------------------------------------------------------- Huber, the solve and the LM loop

def huber(chi2, delta, dsqr):
    """RobustKernelHuber::robustify on arrays: (rho[0], rho[1])"""
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, (2.0 * sq) * delta - dsqr), np.where(inl, 1.0, delta / sq)


def cholesky_solve(H, b, lam):
    """(H + lam I) x = b by Cholesky, n = len(b); None when a pivot is not positive (or NaN)"""
    n = len(b)
    A = [[float(H[i][j]) + (lam if i == j else 0.0) for j in range(n)] for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        s = A[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k]
        if not s > 0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * n
    for i in range(n):
        s = float(b[i])
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s -= L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def levenberg(est, n, iterations, build_system, trial_chi, oplus):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg on the one free
    vertex of n unknowns: (estimate, last trial, trace).  build_system(est) -> (H, b, robust chi2);
    trial_chi(trial) -> robust chi2; oplus(est, x) -> exp(x) * est, and it may change the list x
    in place (VertexSim3Expmap zeroes x[6] under fix_scale), which computeScale then reads.  The
    trace records iterations, rejected, lam (per iteration), trials (per trial: accepted) and
    chi_after (per trial: the robust chi2 of the kept estimate)."""
    tr = SimpleNamespace(iterations=0, rejected=0, lam=[], trials=[], chi_after=[])
    trial = est
    lam = ni = 0.0
    stop_bad = 0
    for it in range(iterations):
        H, b, cur_chi = build_system(est)
        if it == 0:
            max_diag = 0.0
            for j in range(n):  # std::max(fabs(h), maxDiagonal)
                a = abs(float(H[j][j]))
                max_diag = max_diag if a < max_diag else a
            lam = 1e-5 * max_diag
            ni = 2.0
            stop_bad = 0
        tr.iterations += 1
        tr.lam.append(lam)
        ini_chi = cur_chi
        rho = 0.0
        qmax = 0
        while True:
            x = cholesky_solve(H, b, lam)
            ok = x is not None
            if ok:
                trial = oplus(est, x)
                tmp_chi = trial_chi(trial)
            else:  # a rejected zero step
                x = [0.0] * n
                trial = est
                tmp_chi = DBL_MAX
            scale = 0.0
            for j in range(n):
                scale += x[j] * (lam * x[j] + float(b[j]))
            scale += 1e-3
            rho = _div(cur_chi - tmp_chi, scale)
            if rho > 0 and math.isfinite(tmp_chi):
                t3 = 2.0 * rho - 1.0
                alpha = min(1.0 - (t3 * t3) * t3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur_chi = tmp_chi
                est = trial
                tr.trials.append(True)
            else:
                lam *= ni
                ni *= 2.0
                tr.rejected += 1
                tr.trials.append(False)
            tr.chi_after.append(cur_chi)
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
        if (ini_chi - cur_chi) * 1e3 < ini_chi:
            stop_bad += 1
        else:
            stop_bad = 0
        if stop_bad >= 3:
            break
    return est, trial, tr
