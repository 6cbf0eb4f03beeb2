"""CPU restatement of Optimizer::PoseOptimization (src/Optimizer.cpp:291-513)
with the g2o pieces it runs: OptimizationAlgorithmLevenberg::solve
(core/optimization_algorithm_levenberg.cpp:61-189), BaseUnaryEdge::
constructQuadraticForm (core/base_unary_edge.hpp:43-72), RobustKernelHuber
(core/robust_kernel_impl.{h,cpp}), EdgeSE3ProjectXYZOnlyPose /
EdgeStereoSE3ProjectXYZOnlyPose (types/types_six_dof_expmap.cpp:285-385) and
SE3Quat (types/se3quat.h:58-64, 104-110, 217-257, 280-285).

Sequential float64, the float casts where the reference has them: the stereo
projection's invz, Huber's dsqr, the classification's (float)chi2 >
(float)threshold, inputs and the returned pose in float32.  The quaternion
algebra is Eigen 3's as recalled (Quaternion(Matrix3), operator*,
_transformVector, toRotationMatrix, normalize); pow(theta, 3) is written
theta*theta*theta and the dense LDLT is a plain Cholesky whose non-positive
pivot is the failed solve, taken as a rejected zero step.  g2o needs Eigen to
compile, so parity against a g2o build is unpinned.

Per-edge terms are numpy element-wise expressions (one IEEE operation per
numpy call, no fused multiply-add); sums over edges are np.sum; everything
per-trial is Python float arithmetic.  csrc/poseopt.hip writes the same
expressions in the same association order, so the two differ only by the order
in which the edges are summed.
"""
import math
from types import SimpleNamespace

import numpy as np

F32 = np.float32
TH_MONO, TH_STEREO = F32(5.991), F32(7.815)
DELTA_MONO, DELTA_STEREO = float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815)))
DSQR_MONO, DSQR_STEREO = float(F32(DELTA_MONO * DELTA_MONO)), float(F32(DELTA_STEREO * DELTA_STEREO))
DBL_MAX = float(np.finfo(np.float64).max)
UPPER = [(j, k) for j in range(6) for k in range(j, 6)]  # the 21 entries of H


# ---------------------------------------------------------------- SE3Quat: q = (x, y, z, w), t

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


def quat_normalized(q):
    """SE3Quat::normalizeRotation"""
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [_div(v, n) for v in q]


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return float("nan") if a == 0 or a != a else math.copysign(float("inf"), a) * math.copysign(1.0, b)


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


def se3_from_T(T):
    """Converter::toSE3Quat of a float32 [R|t]"""
    T = np.asarray(T, F32)
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    return quat_normalized(quat_from_R(R)), [float(T[r, 3]) for r in range(3)]


def se3_exp(x):
    """SE3Quat::exp(update), update = (omega, upsilon)"""
    om, up = x[:3], x[3:]
    theta = math.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    O = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    O2 = [[(O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if theta < 0.00001:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        a = math.sin(theta) / theta
        b = (1.0 - math.cos(theta)) / (theta * theta)
        c = (theta - math.sin(theta)) / (theta * theta * theta)
        R = [[(I[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(I[i][j] + b * O[i][j]) + c * O2[i][j] for j in range(3)] for i in range(3)]
    t = [(V[i][0] * up[0] + V[i][1] * up[1]) + V[i][2] * up[2] for i in range(3)]
    return quat_normalized(quat_from_R(R)), t


def se3_mul(a, b):
    """SE3Quat::operator*"""
    qa, ta = a
    qb, tb = b
    r = quat_rotate(qa, tb)
    return quat_normalized(quat_mul(qa, qb)), [ta[i] + r[i] for i in range(3)]


def se3_to_T(est):
    q, t = est
    T = np.eye(4)
    T[:3, :3] = quat_to_R(q)
    T[:3, 3] = t
    return T.astype(F32)


# ---------------------------------------------------------------- the edges

def edge_errors(est, Xw, obs, w, K, bf, float_invz=True):
    """computeError of every edge at `est`: (e (n, 3) with e[:, 2] = 0 for a
    monocular edge, chi2 (n), camera-frame point (x, y, z)).  float_invz=False
    keeps the stereo edge's invz in double: not the reference's arithmetic, the
    smooth function the Jacobian test differentiates."""
    q, t = est
    fx, fy, cx, cy = K
    X = Xw.astype(np.float64)
    r = quat_rotate(q, (X[:, 0], X[:, 1], X[:, 2]))
    x, y, z = r[0] + t[0], r[1] + t[1], r[2] + t[2]
    stereo = obs[:, 2] >= 0
    ou, ov, orr = (obs[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        um, vm = (x / z) * fx + cx, (y / z) * fy + cy                     # project2d, double
        # const float invz = 1.0f / trans_xyz[2] on a Vector3d: a double quotient rounded to float once
        invzf = (1.0 / z).astype(F32).astype(np.float64) if float_invz else 1.0 / z
        us, vs = (x * invzf) * fx + cx, (y * invzf) * fy + cy
        rs = us - bf * invzf
        e0 = ou - np.where(stereo, us, um)
        e1 = ov - np.where(stereo, vs, vm)
        e2 = np.where(stereo, orr - rs, 0.0)
        chi2 = e0 * (w * e0) + e1 * (w * e1)
        chi2 = np.where(stereo, chi2 + e2 * (w * e2), chi2)
    return np.stack([e0, e1, e2], 1), chi2, (x, y, z)


def edge_jacobians(p, stereo, K, bf):
    """linearizeOplus: (n, 3, 6), row 2 zero for a monocular edge"""
    x, y, z = p
    fx, fy, _, _ = K
    with np.errstate(all="ignore"):
        invz = 1.0 / z
        invz2 = invz * invz
        J = np.zeros((len(x), 3, 6))
        J[:, 0, 0] = ((x * y) * invz2) * fx
        J[:, 0, 1] = (-(1.0 + (x * x) * invz2)) * fx
        J[:, 0, 2] = (y * invz) * fx
        J[:, 0, 3] = (-invz) * fx
        J[:, 0, 5] = (x * invz2) * fx
        J[:, 1, 0] = (1.0 + (y * y) * invz2) * fy
        J[:, 1, 1] = (((-x) * y) * invz2) * fy
        J[:, 1, 2] = ((-x) * invz) * fy
        J[:, 1, 4] = (-invz) * fy
        J[:, 1, 5] = (y * invz2) * fy
        J[:, 2, 0] = np.where(stereo, J[:, 0, 0] - (bf * y) * invz2, 0.0)
        J[:, 2, 1] = np.where(stereo, J[:, 0, 1] + (bf * x) * invz2, 0.0)
        J[:, 2, 2] = np.where(stereo, J[:, 0, 2], 0.0)
        J[:, 2, 3] = np.where(stereo, J[:, 0, 3], 0.0)
        J[:, 2, 5] = np.where(stereo, J[:, 0, 5] - bf * invz2, 0.0)
    return J


def huber(chi2, stereo):
    """RobustKernelHuber::robustify: (rho[0], rho[1])"""
    delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
    dsqr = np.where(stereo, DSQR_STEREO, DSQR_MONO)
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, (2.0 * sq) * delta - dsqr), np.where(inl, 1.0, delta / sq)


def build_system(est, Xw, obs, w, K, bf, active, robust):
    """computeActiveErrors + activeRobustChi2 + buildSystem over the active
    edges: (H (6, 6), b (6), robust chi2 sum)"""
    Xa, oa, wa = Xw[active], obs[active], w[active]
    stereo = oa[:, 2] >= 0
    e, chi2, p = edge_errors(est, Xa, oa, wa, K, bf)
    J = edge_jacobians(p, stereo, K, bf)
    if robust:
        rho0, rho1 = huber(chi2, stereo)
    else:
        rho0, rho1 = chi2, np.ones_like(chi2)
    with np.errstate(all="ignore"):
        W = rho1 * wa
        H = np.zeros((6, 6))
        for j, k in UPPER:
            c = ((W * J[:, 0, j]) * J[:, 0, k] + (W * J[:, 1, j]) * J[:, 1, k]) + (W * J[:, 2, j]) * J[:, 2, k]
            H[j, k] = H[k, j] = float(np.sum(c))
        we = wa[:, None] * e
        b = np.zeros(6)
        for j in range(6):
            c = rho1 * ((J[:, 0, j] * we[:, 0] + J[:, 1, j] * we[:, 1]) + J[:, 2, j] * we[:, 2])
            b[j] = -float(np.sum(c))
        return H, b, float(np.sum(rho0))


def solve6(H, b, lam):
    """(H + lam I) x = b by Cholesky; None when a pivot is not positive"""
    A = [[float(H[i][j]) + (lam if i == j else 0.0) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k]
        if not s > 0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


# ---------------------------------------------------------------- Optimizer::PoseOptimization

def pose_optimization(Tcw0, Xw, obs, inv_sigma2, K, bf):
    """Tcw0 (3x4 or 4x4), Xw (n, 3), obs (n, 3) = (u, v, uRight; uRight < 0:
    monocular), inv_sigma2 (n), K = (fx, fy, cx, cy), bf -- all taken as
    float32.  Returns a namespace: Tcw (4x4 float32), outlier (n bool), n_good,
    rounds, trace (per round: iterations, rejected, lam (per iteration), trials
    (per trial: accepted), chi_after (per trial: the robust chi2 of the kept
    estimate), chi2 (n float64, what the classification read))."""
    Tcw0 = np.asarray(Tcw0, F32)
    Xw = np.asarray(Xw, F32).reshape(-1, 3)
    obs = np.asarray(obs, F32).reshape(-1, 3)
    w = np.asarray(inv_sigma2, F32).astype(np.float64).reshape(-1)
    K = tuple(float(F32(v)) for v in K)
    bf = float(F32(bf))
    n = len(Xw)
    T0 = np.eye(4, dtype=F32)
    T0[:3] = Tcw0[:3]
    out = SimpleNamespace(Tcw=T0, outlier=np.zeros(n, bool), n_good=0, rounds=0, trace=[])
    if n < 3:
        return out
    stereo = obs[:, 2] >= 0
    thr = np.where(stereo, TH_STEREO, TH_MONO).astype(F32)
    flagged = np.zeros(n, bool)
    n_bad = 0
    est = se3_from_T(Tcw0)
    for it in range(4):
        robust = it < 3
        est = se3_from_T(Tcw0)
        trial = est
        active = ~flagged
        H, b, cur_chi = build_system(est, Xw, obs, w, K, bf, active, robust)
        max_diag = 0.0
        for j in range(6):  # std::max(fabs(h), maxDiagonal)
            a = abs(float(H[j][j]))
            max_diag = max_diag if a < max_diag else a
        lam = 1e-5 * max_diag
        ni = 2.0
        stop_bad = 0
        tr = SimpleNamespace(iterations=0, rejected=0, lam=[], trials=[], chi_after=[], chi2=None)
        for _ in range(10):
            tr.iterations += 1
            tr.lam.append(lam)
            ini_chi = cur_chi
            rho = 0.0
            qmax = 0
            while True:
                x = solve6(H, b, lam)
                ok = x is not None
                if not ok:
                    x = [0.0] * 6
                trial = se3_mul(se3_exp(x), est) if ok else est
                Ht, bt, tmp_chi = build_system(trial, Xw, obs, w, K, bf, active, robust)
                if not ok:
                    tmp_chi = DBL_MAX
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + float(b[j]))
                scale += 1e-3
                rho = _div(cur_chi - tmp_chi, scale)
                if rho > 0 and math.isfinite(tmp_chi):
                    t3 = 2.0 * rho - 1.0
                    alpha = min(1.0 - (t3 * t3) * t3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur_chi = tmp_chi
                    est, H, b = trial, Ht, bt
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
        # classification: active edges keep the error of the last trial, flagged ones are recomputed
        _, chi_trial, _ = edge_errors(trial, Xw, obs, w, K, bf)
        _, chi_est, _ = edge_errors(est, Xw, obs, w, K, bf)
        chi2 = np.where(flagged, chi_est, chi_trial)
        tr.chi2 = chi2
        with np.errstate(all="ignore"):
            flagged = chi2.astype(F32) > thr
        n_bad = int(flagged.sum())
        out.trace.append(tr)
        out.rounds = it + 1
        if n < 10:
            break
    out.Tcw = se3_to_T(est)
    out.outlier = flagged
    out.n_good = n - n_bad
    return out


def threshold_margin(result, obs):
    """smallest relative distance of a classification chi2 from its threshold
    over all rounds (inf when no round ran)"""
    obs = np.asarray(obs, F32).reshape(-1, 3)
    thr = np.where(obs[:, 2] >= 0, float(TH_STEREO), float(TH_MONO))
    m = float("inf")
    for tr in result.trace:
        m = min(m, float(np.min(np.abs(tr.chi2 - thr) / thr)))
    return m
