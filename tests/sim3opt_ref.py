"""CPU restatement of Optimizer::OptimizeSim3 (src/Optimizer.cpp:1229-1433)
with the g2o pieces it runs: EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ and
VertexSim3Expmap (types/types_seven_dof_expmap.h:61-90, 131-172), Sim3
(types/sim3.h:70-146, 233-236, 266-272), the numeric Jacobians of
BaseBinaryEdge::linearizeOplus and the robust branch of constructQuadraticForm
(core/base_binary_edge.hpp:131-204, 91-113), RobustKernelHuber
(core/robust_kernel_impl.{h,cpp}) and OptimizationAlgorithmLevenberg::solve
(core/optimization_algorithm_levenberg.cpp:61-189).

Sequential float64; inputs, th2, Huber's delta and dsqr and the returned T12 in
float32 where the reference has them.  The quaternion helpers, the dense solve
and the Levenberg-Marquardt loop are tests/lm_ref.py's, shared with
poseopt_ref.py; a failed solve is taken as a rejected zero step.  g2o needs
Eigen to compile, so parity against a g2o build is unpinned.

Per-edge terms are numpy element-wise expressions (one IEEE operation per
numpy call, no fused multiply-add); sums over edges are np.sum; everything
per-trial is Python float arithmetic.  csrc/sim3opt.hip writes the same
expressions in the same association order, so the two differ only by the order
in which the edges are summed (and by exp / sin / cos, which come from libm
here and from the device library there).
"""
import math
from types import SimpleNamespace

import numpy as np

from lm_ref import _div, huber, levenberg, quat_from_R, quat_mul, quat_rotate, quat_to_R

F32 = np.float32
DELTA = 1e-9                  # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA)    # :148
UPPER = [(j, k) for j in range(7) for k in range(j, 7)]  # the 28 entries of H


# ---------------------------------------------------------------- Sim3: (q = (x, y, z, w), t, s)

def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return float("inf")


def sim3_exp(u):
    """Sim3(const Vector7d& update), update = (omega, upsilon, sigma)"""
    om, up, sigma = u[0:3], u[3:6], u[6]
    theta = math.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    O = [[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]
    s = _exp(sigma)
    O2 = [[(O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    eps = 0.00001

    def rodrigues():
        a = math.sin(theta) / theta
        b = (1.0 - math.cos(theta)) / (theta * theta)
        return [[(I[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]

    def small():
        return [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]

    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A = 1.0 / 2.0
            B = 1.0 / 6.0
            R = small()
        else:
            theta2 = theta * theta
            A = (1.0 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            R = rodrigues()
    else:
        C = (s - 1.0) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
            R = small()
        else:
            R = rodrigues()
            a = s * math.sin(theta)
            b = s * math.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2
    q = quat_from_R(R)  # not normalised
    W = [[(A * O[i][j] + B * O2[i][j]) + C * I[i][j] for j in range(3)] for i in range(3)]
    t = [(W[i][0] * up[0] + W[i][1] * up[1]) + W[i][2] * up[2] for i in range(3)]
    return q, t, s


def sim3_mul(a, b):
    """Sim3::operator*: the quaternion product is not normalised"""
    qa, ta, sa = a
    qb, tb, sb = b
    r = quat_rotate(qa, tb)
    return quat_mul(qa, qb), [sa * r[i] + ta[i] for i in range(3)], sa * sb


def sim3_inverse(a):
    q, t, s = a
    qc = [-q[0], -q[1], -q[2], q[3]]
    c = _div(-1.0, s)
    r = quat_rotate(qc, (c * t[0], c * t[1], c * t[2]))
    return qc, [r[0], r[1], r[2]], _div(1.0, s)


def sim3_map(S, P):
    """Sim3::map on P = (x, y, z) arrays"""
    q, t, s = S
    r = quat_rotate(q, P)
    return s * r[0] + t[0], s * r[1] + t[1], s * r[2] + t[2]


def oplus(S, u, fix_scale):
    """VertexSim3Expmap::oplusImpl"""
    u = list(u)
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def sim3_to_T(S):
    """Converter::toCvMat(g2o::Sim3): [sR t; 0 1] in float32"""
    q, t, s = S
    R = quat_to_R(q)
    T = np.eye(4)
    for i in range(3):
        for j in range(3):
            T[i, j] = s * R[i][j]
        T[i, 3] = t[i]
    with np.errstate(all="ignore"):
        return T.astype(F32)


# ---------------------------------------------------------------- the edges

def problem(P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2):
    """the correspondences as the library takes them (float32), widened"""
    f = lambda a, w: np.asarray(a, F32).reshape(-1, w).astype(np.float64)
    p = SimpleNamespace(P1=f(P1c, 3), P2=f(P2c, 3), o1=f(obs1, 2), o2=f(obs2, 2), w1=f(inv_sigma2_1, 1)[:, 0],
                        w2=f(inv_sigma2_2, 1)[:, 0], K1=tuple(float(F32(v)) for v in K1),
                        K2=tuple(float(F32(v)) for v in K2))
    p.n = len(p.P1)
    return p


def take(p, idx):
    return SimpleNamespace(P1=p.P1[idx], P2=p.P2[idx], o1=p.o1[idx], o2=p.o2[idx], w1=p.w1[idx], w2=p.w2[idx],
                           K1=p.K1, K2=p.K2, n=len(p.P1[idx]))


def _project_error(S, P, obs, K):
    x, y, z = sim3_map(S, (P[:, 0], P[:, 1], P[:, 2]))
    with np.errstate(all="ignore"):
        return obs[:, 0] - ((x / z) * K[0] + K[2]), obs[:, 1] - ((y / z) * K[1] + K[3])


def edge_errors(S, p, Sinv=None):
    """computeError of both edges of every correspondence at S: (e12 (2 arrays),
    e21 (2 arrays), chi2 of e12, chi2 of e21)"""
    if Sinv is None:
        Sinv = sim3_inverse(S)
    e12 = _project_error(S, p.P2, p.o1, p.K1)
    e21 = _project_error(Sinv, p.P1, p.o2, p.K2)
    with np.errstate(all="ignore"):
        c12 = e12[0] * (p.w1 * e12[0]) + e12[1] * (p.w1 * e12[1])
        c21 = e21[0] * (p.w2 * e21[0]) + e21[1] * (p.w2 * e21[1])
    return e12, e21, c12, c21


def numeric_jacobians(S, p, fix_scale):
    """BaseBinaryEdge::linearizeOplus: J12, J21 as lists of 7 columns, each (2 arrays)"""
    J12, J21 = [], []
    for d in range(7):
        u = [0.0] * 7
        u[d] = DELTA
        ep12, ep21, _, _ = edge_errors(oplus(S, u, fix_scale), p)
        u[d] = -DELTA
        em12, em21, _, _ = edge_errors(oplus(S, u, fix_scale), p)
        with np.errstate(all="ignore"):
            J12.append((SCALAR * (ep12[0] - em12[0]), SCALAR * (ep12[1] - em12[1])))
            J21.append((SCALAR * (ep21[0] - em21[0]), SCALAR * (ep21[1] - em21[1])))
    return J12, J21


def _interleaved_sum(a, b):
    """sum over the edges in the graph's order: e12, e21 of each correspondence in turn"""
    return float(np.sum(np.stack([a, b], 1).reshape(-1)))


def robust_chi2(S, p, delta, dsqr):
    _, _, c12, c21 = edge_errors(S, p)
    return _interleaved_sum(huber(c12, delta, dsqr)[0], huber(c21, delta, dsqr)[0])


def build_system(S, p, fix_scale, delta, dsqr):
    """computeActiveErrors + activeRobustChi2 + buildSystem: (H (7, 7), b (7), robust chi2 sum)"""
    e12, e21, c12, c21 = edge_errors(S, p)
    J12, J21 = numeric_jacobians(S, p, fix_scale)
    H = np.zeros((7, 7))
    b = np.zeros(7)
    with np.errstate(all="ignore"):
        terms = []
        for e, c, J, w in ((e12, c12, J12, p.w1), (e21, c21, J21, p.w2)):
            rho0, rho1 = huber(c, delta, dsqr)
            W = rho1 * w
            omr = ((-(w * e[0])) * rho1, (-(w * e[1])) * rho1)
            terms.append((rho0, W, omr, J))
        for j, k in UPPER:
            c = [(W * J[j][0]) * J[k][0] + (W * J[j][1]) * J[k][1] for _, W, _, J in terms]
            H[j, k] = H[k, j] = _interleaved_sum(c[0], c[1])
        for j in range(7):
            c = [J[j][0] * omr[0] + J[j][1] * omr[1] for _, _, omr, J in terms]
            b[j] = _interleaved_sum(c[0], c[1])
        return H, b, _interleaved_sum(terms[0][0], terms[1][0])


def optimize(est, p, iterations, fix_scale, delta, dsqr):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg
    on the one free vertex: (estimate, last trial, trace)"""
    def step(S, x):
        if fix_scale:
            x[6] = 0.0  # oplusImpl zeroes the solver's own x[6] through its const_cast: computeScale sees it
        return oplus(S, x, fix_scale)
    return levenberg(est, 7, iterations, lambda S: build_system(S, p, fix_scale, delta, dsqr),
                     lambda S: robust_chi2(S, p, delta, dsqr), step)


# ---------------------------------------------------------------- Optimizer::OptimizeSim3

def optimize_sim3(q12, t12, s12, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2, fix_scale):
    """Returns a namespace: S = (q, t, s) (the input objects when the reference
    does not write g2oS12), T12 (4x4 float32), removed (n bool), n_in, rounds,
    n_bad_first, trace (per optimisation), chi2 (per check: the n x 2 chi2 it
    read, NaN where the pair was no longer in the graph)."""
    p = problem(P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2)
    S0 = ([float(v) for v in q12], [float(v) for v in t12], float(s12))
    th2 = float(F32(th2))
    delta = float(F32(math.sqrt(th2)))       # const float deltaHuber = sqrt(th2)
    dsqr = float(F32(delta * delta))         # robust_kernel_impl.h:85: float dsqr
    fix_scale = bool(fix_scale)
    n = p.n
    out = SimpleNamespace(S=S0, T12=sim3_to_T(S0), removed=np.zeros(n, bool), n_in=0, rounds=0, n_bad_first=0,
                          trace=[], chi2=[])
    if n == 0:
        return out
    est, trial, tr = optimize(S0, p, 5, fix_scale, delta, dsqr)
    out.trace.append(tr)
    out.rounds = 1
    _, _, c12, c21 = edge_errors(trial, p)
    out.chi2.append(np.stack([c12, c21], 1))
    with np.errstate(all="ignore"):
        bad = (c12 > th2) | (c21 > th2)
    out.removed = bad.copy()
    n_bad = int(bad.sum())
    out.n_bad_first = n_bad
    more = 10 if n_bad > 0 else 5
    if n - n_bad < 10:
        return out
    keep = np.nonzero(~bad)[0]
    est, trial, tr = optimize(est, take(p, keep), more, fix_scale, delta, dsqr)
    out.trace.append(tr)
    out.rounds = 2
    _, _, c12, c21 = edge_errors(trial, take(p, keep))
    chi = np.full((n, 2), np.nan)
    chi[keep, 0], chi[keep, 1] = c12, c21
    out.chi2.append(chi)
    with np.errstate(all="ignore"):
        bad2 = (c12 > th2) | (c21 > th2)
    out.removed[keep[bad2]] = True
    out.n_in = int((~bad2).sum())
    out.S = est
    out.T12 = sim3_to_T(est)
    return out


def threshold_margin(result, th2):
    """smallest relative distance of a chi2 either check read from th2 (inf when none ran)"""
    th2 = float(F32(th2))
    m = float("inf")
    for chi in result.chi2:
        c = chi[np.isfinite(chi)]
        if len(c):
            m = min(m, float(np.min(np.abs(c - th2) / th2)))
    return m
