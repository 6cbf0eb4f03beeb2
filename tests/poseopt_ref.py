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
algebra, the dense solve and the Levenberg-Marquardt loop are tests/lm_ref.py's,
shared with sim3opt_ref.py; pow(theta, 3) is written theta*theta*theta and a
failed solve is taken as a rejected zero step.  g2o needs Eigen to compile, so
parity against a g2o build is unpinned.

Per-edge terms are numpy element-wise expressions (one IEEE operation per
numpy call, no fused multiply-add); sums over edges are np.sum; everything
per-trial is Python float arithmetic.  csrc/poseopt.hip writes the same
expressions in the same association order, so the two differ only by the order
in which the edges are summed.
"""
import math
from types import SimpleNamespace

import numpy as np

import lm_ref
from lm_ref import _div, levenberg, quat_from_R, quat_mul, quat_rotate, quat_to_R  # noqa: F401 (re-exported)

F32 = np.float32
TH_MONO, TH_STEREO = F32(5.991), F32(7.815)
DELTA_MONO, DELTA_STEREO = float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815)))
DSQR_MONO, DSQR_STEREO = float(F32(DELTA_MONO * DELTA_MONO)), float(F32(DELTA_STEREO * DELTA_STEREO))
UPPER = [(j, k) for j in range(6) for k in range(j, 6)]  # the 21 entries of H


# ---------------------------------------------------------------- SE3Quat: q = (x, y, z, w), t

def quat_normalized(q):
    """SE3Quat::normalizeRotation"""
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [_div(v, n) for v in q]


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
    """RobustKernelHuber::robustify with the edge type's delta: (rho[0], rho[1])"""
    return lm_ref.huber(chi2, np.where(stereo, DELTA_STEREO, DELTA_MONO), np.where(stereo, DSQR_STEREO, DSQR_MONO))


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
        active = ~flagged
        build = lambda e: build_system(e, Xw, obs, w, K, bf, active, robust)
        # the kernel takes an accepted trial's system from the trial pass; building it again at the
        # same estimate gives the same bits
        est, trial, tr = levenberg(est, 6, 10, build, lambda t: build(t)[2], lambda e, x: se3_mul(se3_exp(x), e))
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
