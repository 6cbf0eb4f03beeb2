"""CPU restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:905-1200)
from the optimisation on (the vertex and edge enumeration and the write-back
are the adapter's, include/orbslam2_amd/EssentialGraphOptimizer.h), with the
g2o pieces it runs: VertexSim3Expmap and EdgeSim3
(types/types_seven_dof_expmap.h:61-70, 107-115), Sim3 with its log
(types/sim3.h:64-67, 70-146, 148-230, 233-236, 266-272; se3_ops.hpp:27-47), the
numeric Jacobians of both ends (core/base_binary_edge.hpp:131-205), the
non-robust quadratic form (:75-90), the active set of initializeOptimization(0)
(core/sparse_optimizer.cpp:206-260) and OptimizationAlgorithmLevenberg::solve
(core/optimization_algorithm_levenberg.cpp:61-189) started from
setUserLambdaInit(1e-16).  csrc/essential.hip writes the same expressions in
the same association order and adds every sum in the same order.

Everything is float64.  A batch of Sim3s is a list of eight arrays (qx, qy, qz,
qw, tx, ty, tz, s); every expression is a numpy element-wise operation (one IEEE
operation per call, no fused multiply-add), a branch is both sides computed
and selected, so an element's bits are those of the scalar code.  Sums over
edges and vertices are sequential in the kernel's order.  exp, log, sin, cos and
acos are callables of a `Fn`, so that a run can move their results (nudged).

Deviations, as globalba_ref states its own: Omega = I dropped from the error's
chi2 and the quadratic form; the products are associated as written here;
W.lu().solve(t) is a 3x3 elimination with partial pivoting (the first largest
|entry| of the column) in this file's order; the system (H + lambda I) x = b over
the free active vertices in ascending index is solved by the dense Cholesky of
globalba_ref.blocked_order_solve in place of Eigen's sparse solver; a pivot that
is not positive (or NaN) is the failed solve and a failed solve is a rejected
zero step; parity against a g2o build is unpinned (g2o needs Eigen).
"""
import math
from types import SimpleNamespace

import numpy as np

from globalba_ref import blocked_order_solve
from lm_ref import DBL_MAX, _div, quat_mul, quat_rotate, quat_to_R

F32 = np.float32
DELTA = 1e-9                  # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA)    # :148
EPS = 0.00001                 # sim3.h:90, :165
ONE_MINUS_EPS = 1.0 - EPS
LAMBDA_INIT = 1e-16           # Optimizer.cpp:922
THREADS = 256                 # csrc/essential.hip: kThreads, the lanes whose values one chi2 / scale slot adds


def _libm(f, npf):
    """libm's scalar function element by element (numpy's own loops differ from it in the last bit on
    some CPUs, so the restatement does not use them); numpy's for an argument outside the domain and for
    the complex arguments of the tests' complex-step derivative"""
    def one(v):
        try:
            return f(v)
        except (ValueError, OverflowError):
            with np.errstate(all="ignore"):
                return float(npf(np.float64(v)))
    each = np.frompyfunc(one, 1, 1)

    def g(x):
        x = np.asarray(x)
        return npf(x) if np.iscomplexobj(x) else np.asarray(each(x.astype(np.float64)), dtype=np.float64)
    return g


LIBM = {"exp": _libm(math.exp, np.exp), "log": _libm(math.log, np.log), "sin": _libm(math.sin, np.sin),
        "cos": _libm(math.cos, np.cos), "acos": _libm(math.acos, np.arccos)}


class Fn:
    """the five library functions of the arithmetic, and the margins of every branch decided with them"""

    def __init__(self):
        self.margins = []

    exp = staticmethod(LIBM["exp"])
    log = staticmethod(LIBM["log"])
    sin = staticmethod(LIBM["sin"])
    cos = staticmethod(LIBM["cos"])
    acos = staticmethod(LIBM["acos"])

    def note(self, value, threshold):
        """a branch compared `value` with `threshold`: its relative distance"""
        m = np.abs(np.real(value) - threshold) / abs(threshold)
        m = m[np.isfinite(m)]
        if m.size:
            self.margins.append(float(m.min()))


class NudgedFn(Fn):
    """every result of the five functions moved by up to `ulps` ulp, by an amount that is a seeded hash
    of the argument's bits: another library's function, which like it gives one result per argument (the
    two sides of a central difference see the same function).  A result that is exact at an exact
    argument (exp, sin, cos of 0; log, acos of 1) stays: the device library's functions are exact there too"""

    def __init__(self, seed, ulps=2):
        super().__init__()
        self.ulps = ulps
        for k, (name, exact_at) in enumerate((("exp", 0.0), ("log", 1.0), ("sin", 0.0), ("cos", 0.0), ("acos", 1.0))):
            setattr(self, name, self._nudged(LIBM[name], exact_at,
                                             np.uint64(0x9E3779B97F4A7C15 * (5 * seed + k + 1) % 2 ** 64)))

    def _nudged(self, f, exact_at, salt):
        span = np.uint64(2 * self.ulps + 1)

        def g(x):
            x = np.asarray(x, np.float64)
            r = np.array(f(x), np.float64)
            with np.errstate(over="ignore"):
                h = (x.view(np.uint64) ^ salt) * np.uint64(0xD6E8FEB86659FD93)
                h = (h ^ (h >> np.uint64(32))) * np.uint64(0xD6E8FEB86659FD93)
                k = ((h >> np.uint64(40)) % span).astype(np.int64) - self.ulps
            move = np.isfinite(r) & (r != 0) & (x != exact_at)
            bits = r.view(np.int64) + np.where(move, k, 0)  # k ulp along the magnitude
            return bits.view(np.float64)
        return g


def _ignore(f):
    def g(*a, **kw):
        with np.errstate(all="ignore"):
            return f(*a, **kw)
    g.__doc__ = f.__doc__
    return g


# ---------------------------------------------------------------- Sim3 on batches

def quat_from_R(R):
    """lm_ref.quat_from_R (Eigen: Quaterniond(Matrix3d), not normalised) on arrays: the four branches
    computed, one selected"""
    t = (R[0][0] + R[1][1]) + R[2][2]
    s = np.sqrt(t + 1.0)
    h = 0.5 / s
    out = [[(R[2][1] - R[1][2]) * h, (R[0][2] - R[2][0]) * h, (R[1][0] - R[0][1]) * h, 0.5 * s]]
    for i in range(3):
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = np.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
        h = 0.5 / s
        q = [None] * 4
        q[i] = 0.5 * s
        q[3] = (R[k][j] - R[j][k]) * h
        q[j] = (R[j][i] + R[i][j]) * h
        q[k] = (R[k][i] + R[i][k]) * h
        out.append(q)
    i1 = R[1][1] > R[0][0]
    i2 = R[2][2] > np.where(i1, R[1][1], R[0][0])
    which = np.where(t > 0, 0, np.where(i2, 3, np.where(i1, 2, 1)))
    return [np.choose(which, [out[b][c] for b in range(4)]) for c in range(4)]


def _skew(om):
    z = np.zeros_like(om[0])
    return [[z, -om[2], om[1]], [om[2], z, -om[0]], [-om[1], om[0], z]]


def _matmul3(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


@_ignore
def sim3_exp(u, fn):
    """Sim3(const Vector7d& update) as sim3opt_ref.sim3_exp has it, on a batch u = 7 arrays"""
    om, up, sigma = u[0:3], u[3:6], u[6]
    theta = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    O = _skew(om)
    s = fn.exp(sigma)
    O2 = _matmul3(O, O)
    eye = lambda i, j: 1.0 if i == j else 0.0
    small_sigma = np.abs(sigma) < EPS
    small_theta = theta < EPS
    fn.note(np.abs(sigma), EPS)
    fn.note(theta, EPS)
    sn, cs = fn.sin(theta), fn.cos(theta)
    ra = sn / theta
    rb = (1.0 - cs) / (theta * theta)
    R = [[np.where(small_theta, (eye(i, j) + O[i][j]) + O2[i][j], (eye(i, j) + ra * O[i][j]) + rb * O2[i][j])
          for j in range(3)] for i in range(3)]
    theta2 = theta * theta
    sigma2 = sigma * sigma
    C = np.where(small_sigma, 1.0, (s - 1.0) / sigma)
    a = s * sn
    b = s * cs
    c = theta2 + sigma2
    A = np.where(small_sigma,
                 np.where(small_theta, 1.0 / 2.0, (1.0 - cs) / theta2),
                 np.where(small_theta, ((sigma - 1.0) * s + 1.0) / sigma2, (a * sigma + (1.0 - b) * theta) / (theta * c)))
    B = np.where(small_sigma,
                 np.where(small_theta, 1.0 / 6.0, (theta - sn) / (theta2 * theta)),
                 np.where(small_theta, (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma),
                          ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2))
    q = quat_from_R(R)
    W = [[(A * O[i][j] + B * O2[i][j]) + C * eye(i, j) for j in range(3)] for i in range(3)]
    t = [(W[i][0] * up[0] + W[i][1] * up[1]) + W[i][2] * up[2] for i in range(3)]
    return q + t + [s + np.zeros_like(theta)]


def _lu_solve3(W, t):
    """W x = t by elimination with partial pivoting, the first largest |entry| of the column"""
    M = np.stack([np.stack([W[i][0], W[i][1], W[i][2], t[i]]) for i in range(3)])  # (3, 4, n)
    n = M.shape[2]
    col = np.arange(n)
    a = np.abs(M[:, 0, :])
    p1 = a[1] > a[0]
    p2 = a[2] > np.where(p1, a[1], a[0])
    best = np.where(p2, 2, np.where(p1, 1, 0))
    perm = np.tile(np.arange(3)[:, None], (1, n))
    perm[0] = best
    perm[best, col] = 0
    M = M[perm, :, col[None, :]].transpose(0, 2, 1)  # rows permuted per element
    for r in (1, 2):
        f = M[r, 0] / M[0, 0]
        for c in (1, 2, 3):
            M[r, c] = M[r, c] - f * M[0, c]
    swap = np.abs(M[2, 1]) > np.abs(M[1, 1])
    r1 = np.where(swap, M[2], M[1])
    r2 = np.where(swap, M[1], M[2])
    f = r2[1] / r1[1]
    r22 = r2[2] - f * r1[2]
    r23 = r2[3] - f * r1[3]
    x2 = r23 / r22
    x1 = (r1[3] - r1[2] * x2) / r1[1]
    x0 = ((M[0, 3] - M[0, 1] * x1) - M[0, 2] * x2) / M[0, 0]
    return [x0, x1, x2]


@_ignore
def sim3_log(S, fn):
    """Sim3::log (sim3.h:148-230) as written, on a batch: 7 arrays (omega, upsilon, sigma)"""
    q, t, s = S[0:4], S[4:7], S[7]
    sigma = fn.log(s)
    R = quat_to_R(q)
    d = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1.0)
    small_sigma = np.abs(sigma) < EPS
    near = d > ONE_MINUS_EPS
    fn.note(np.abs(sigma), EPS)
    fn.note(d, ONE_MINUS_EPS)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    theta = fn.acos(d)
    theta2 = theta * theta
    k = theta / (2.0 * np.sqrt(1.0 - d * d))
    omega = [np.where(near, 0.5 * dR[i], k * dR[i]) for i in range(3)]
    O = _skew(omega)
    sn, cs = fn.sin(theta), fn.cos(theta)
    sigma2 = sigma * sigma
    C = np.where(small_sigma, 1.0, (s - 1.0) / sigma)
    a = s * sn
    b = s * cs
    c = theta2 + sigma * sigma
    A = np.where(small_sigma,
                 np.where(near, 1.0 / 2.0, (1.0 - cs) / theta2),
                 np.where(near, ((sigma - 1.0) * s + 1.0) / sigma2, (a * sigma + (1.0 - b) * theta) / (theta * c)))
    B = np.where(small_sigma,
                 np.where(near, 1.0 / 6.0, (theta - sn) / (theta2 * theta)),
                 np.where(near, (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma),
                          ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2))
    BO = [[B * O[i][j] for j in range(3)] for i in range(3)]
    BOO = _matmul3(BO, O)
    eye = lambda i, j: 1.0 if i == j else 0.0
    W = [[(A * O[i][j] + BOO[i][j]) + C * eye(i, j) for j in range(3)] for i in range(3)]
    upsilon = _lu_solve3(W, t)
    return omega + upsilon + [sigma]


@_ignore
def sim3_mul(a, b):
    """Sim3::operator*: the quaternion product is not normalised"""
    r = quat_rotate(a[0:4], b[4:7])
    return quat_mul(a[0:4], b[0:4]) + [a[7] * r[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


@_ignore
def sim3_inverse(a):
    qc = [-a[0], -a[1], -a[2], a[3]]
    c = -1.0 / a[7]
    r = quat_rotate(qc, (c * a[4], c * a[5], c * a[6]))
    return qc + [r[0], r[1], r[2]] + [1.0 / a[7]]


@_ignore
def sim3_map(S, P):
    """Sim3::map: s * (r * xyz) + t"""
    r = quat_rotate(S[0:4], P)
    return [S[7] * r[i] + S[4 + i] for i in range(3)]


def take(S, idx):
    return [np.asarray(c)[idx] for c in S]


def as_batch(rows):
    """(n, 8) doubles -> a batch"""
    rows = np.asarray(rows, np.float64).reshape(-1, 8)
    return [rows[:, c].copy() for c in range(8)]


def as_rows(S):
    return np.stack([np.asarray(c, np.float64) for c in S], 1) if len(S[0]) else np.zeros((0, 8))


@_ignore
def oplus(S, u, fix_scale, fn):
    """VertexSim3Expmap::oplusImpl on a batch: Sim3(u) * estimate, u[6] = 0 under fix_scale"""
    u = [np.asarray(c, np.result_type(c, np.float64)) for c in u]
    if fix_scale:
        u[6] = np.zeros_like(u[6])
    return sim3_mul(sim3_exp(u, fn), S)


@_ignore
def edge_error(C, Si, Sj_inv, fn):
    """EdgeSim3::computeError: (C * v1.estimate() * v2.estimate().inverse()).log()"""
    return sim3_log(sim3_mul(sim3_mul(C, Si), Sj_inv), fn)


@_ignore
def chi2_of(e):
    c = e[0] * e[0]
    for k in range(1, 7):
        c = c + e[k] * e[k]
    return c


def slot_sum(values):
    """the sum of one value per lane as the kernels add it: per workgroup of THREADS lanes 16 lanes add
    16 values each in lane order, one lane the 16 sums; the workgroups' sums in workgroup order"""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        return 0.0
    pad = (-v.size) % THREADS
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, 16, 16)
    with np.errstate(all="ignore"):
        rows = v[:, :, 0].copy()
        for k in range(1, 16):
            rows = rows + v[:, :, k]
        tot = rows[:, 0].copy()
        for k in range(1, 16):
            tot = tot + rows[:, k]
        s = float(tot[0])
        for k in range(1, len(tot)):
            s += float(tot[k])
    return s


# ---------------------------------------------------------------- the problem

def make_job(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j, edge_kind, Xw,
             point_ref, fix_scale):
    """the arrays as the library takes them, the vertices' vScw and every edge's measurement"""
    T = np.asarray(Tcw, F32)
    n = len(T)
    T = T.reshape(n, -1, 4)[:, :3].astype(np.float64) if n else np.zeros((0, 3, 4))
    j = SimpleNamespace(n=n, fix_scale=bool(fix_scale))
    j.has_c = np.asarray(has_corrected, np.uint8).reshape(-1) != 0
    j.has_nc = np.asarray(has_noncorrected, np.uint8).reshape(-1) != 0
    j.fixed = np.asarray(fixed, np.uint8).reshape(-1) != 0
    j.ei = np.asarray(edge_i, np.int64).reshape(-1)
    j.ej = np.asarray(edge_j, np.int64).reshape(-1)
    j.kind = np.asarray(edge_kind, np.uint8).reshape(-1)
    j.E = len(j.ei)
    j.Xw = np.asarray(Xw, F32).reshape(-1, 3)
    j.ref = np.asarray(point_ref, np.int64).reshape(-1)
    Sc, Snc = as_batch(Scorrected), as_batch(Snoncorrected)
    # g2o::Sim3(Rcw, tcw, 1.0): Quaterniond(Matrix3d), not normalised
    R = [[T[:, r, c] for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        q = quat_from_R(R) if n else [np.zeros(0)] * 4
    own = q + [T[:, r, 3] for r in range(3)] + [np.ones(n)]
    j.vScw = [np.where(j.has_c, Sc[c], own[c]) for c in range(8)]
    nc = [np.where(j.has_nc, Snc[c], j.vScw[c]) for c in range(8)]
    # kind 0 (LoopConnections): vScw[j] * vScw[i].inverse(); kind 1: the non-corrected Sim3 where there is one
    k0 = j.kind == 0
    Si = [np.where(k0, a[j.ei], b[j.ei]) for a, b in zip(j.vScw, nc)]
    Sj = [np.where(k0, a[j.ej], b[j.ej]) for a, b in zip(j.vScw, nc)]
    j.meas = sim3_mul(Sj, sim3_inverse(Si))
    # initializeOptimization(0): an edge both of whose ends are fixed is not active
    j.e_active = ~(j.fixed[j.ei] & j.fixed[j.ej])
    j.v_active = np.zeros(n, bool)
    j.v_active[j.ei[j.e_active]] = True
    j.v_active[j.ej[j.e_active]] = True
    j.free = j.v_active & ~j.fixed
    j.hlist = np.nonzero(j.free)[0]
    j.hidx = np.full(n, -1)
    j.hidx[j.hlist] = np.arange(len(j.hlist))
    j.nf = len(j.hlist)
    j.ae = np.nonzero(j.e_active)[0]  # ascending edge index
    return j


def active_chi2(est, job, fn):
    """computeActiveErrors: (per-edge errors of the active edges, chi2 per edge over all edges with 0 at
    an inactive one, their sum in the kernel's order)"""
    ae = job.ae
    chi = np.zeros(job.E)
    if len(ae) == 0:
        return [np.zeros(0)] * 7, chi, 0.0
    inv = sim3_inverse(est)
    e = edge_error(take(job.meas, ae), take(est, job.ei[ae]), take(inv, job.ej[ae]), fn)
    chi[ae] = chi2_of(e)
    return e, chi, slot_sum(chi)


def jacobians(est, job, fn):
    """BaseBinaryEdge::linearizeOplus of the active edges: A, B (n_active, 7 rows, 7 columns); the columns
    of a fixed end are zero and never read"""
    ae = job.ae
    vi, vj = job.ei[ae], job.ej[ae]
    C = take(job.meas, ae)
    inv = sim3_inverse(est)
    Si, Sj_inv = take(est, vi), take(inv, vj)
    A = np.zeros((len(ae), 7, 7))
    B = np.zeros((len(ae), 7, 7))
    fi, fj = ~job.fixed[vi], ~job.fixed[vj]
    for d in range(7):
        cols = []
        for sign in (1.0, -1.0):
            u = [np.zeros(job.n) for _ in range(7)]
            u[d] = u[d] + sign * DELTA
            P = oplus(est, u, job.fix_scale, fn)   # the perturbed estimate of every vertex
            Pinv = sim3_inverse(P)
            cols.append((edge_error(C, take(P, vi), Sj_inv, fn), edge_error(C, Si, take(Pinv, vj), fn)))
        with np.errstate(all="ignore"):
            for r in range(7):
                A[:, r, d] = np.where(fi, (cols[0][0][r] - cols[1][0][r]) * SCALAR, 0.0)
                B[:, r, d] = np.where(fj, (cols[0][1][r] - cols[1][1][r]) * SCALAR, 0.0)
    return A, B


@_ignore
def _atb(A, B):
    """per edge A^T B, every entry the sum over the 7 rows in ascending order"""
    out = A[:, 0, :, None] * B[:, 0, None, :]
    for k in range(1, 7):
        out = out + A[:, k, :, None] * B[:, k, None, :]
    return out


@_ignore
def _atv(A, v):
    out = A[:, 0, :] * v[0][:, None]
    for k in range(1, 7):
        out = out + A[:, k, :] * v[k][:, None]
    return out


def build_system(est, job, fn):
    """computeActiveErrors + buildSystem: a namespace with chi (the sum), chi_e, the per-edge blocks, H
    (7 nf square, without lambda) and b, every sum over a vertex's or a pair's edges in ascending edge
    index"""
    e, chi_e, chi = active_chi2(est, job, fn)
    n = 7 * job.nf
    sys = SimpleNamespace(chi=chi, chi_e=chi_e, H=np.zeros((n, n)), b=np.zeros(n), A=None, B=None)
    if len(job.ae) == 0:
        return sys
    A, B = jacobians(est, job, fn)
    sys.A, sys.B = A, B
    me = [-c for c in e]
    AtA, AtB, BtB = _atb(A, A), _atb(A, B), _atb(B, B)
    Atb, Btb = _atv(A, me), _atv(B, me)
    H, b = sys.H, sys.b
    with np.errstate(all="ignore"):
        for k, edge in enumerate(job.ae):  # ascending edge index: each entry's owner adds in this order
            hi, hj = job.hidx[job.ei[edge]], job.hidx[job.ej[edge]]
            if hi >= 0:
                H[7 * hi:7 * hi + 7, 7 * hi:7 * hi + 7] += AtA[k]
                b[7 * hi:7 * hi + 7] += Atb[k]
            if hj >= 0:
                H[7 * hj:7 * hj + 7, 7 * hj:7 * hj + 7] += BtB[k]
                b[7 * hj:7 * hj + 7] += Btb[k]
            if hi >= 0 and hj >= 0:
                H[7 * hi:7 * hi + 7, 7 * hj:7 * hj + 7] += AtB[k]
                H[7 * hj:7 * hj + 7, 7 * hi:7 * hi + 7] += AtB[k].T
    return sys


def solve(sys, lam):
    """(H + lambda I) x = b in blocked_order_solve's order; None for the failed solve"""
    n = len(sys.b)
    S = sys.H.copy()
    with np.errstate(all="ignore"):
        S[np.arange(n), np.arange(n)] = S[np.arange(n), np.arange(n)] + lam
    sol = blocked_order_solve(S, sys.b)
    return None if sol is None else sol[0]


def step(est, x, job, fn):
    """oplus of every free active vertex: (trial estimates, computeScale's per-vertex terms over all
    vertices); x[6] of a vertex is zeroed under fix_scale, as oplusImpl zeroes the solver's"""
    xs = x.reshape(job.nf, 7).copy()
    if job.fix_scale:
        xs[:, 6] = 0.0
    u = [np.zeros(job.n) for _ in range(7)]
    for k in range(7):
        u[k][job.hlist] = xs[:, k]
    moved = oplus(est, u, job.fix_scale, fn)
    trial = [np.where(job.free, m, c) for m, c in zip(moved, est)]
    return trial, xs


def scale_sum(xs, sys, lam, job):
    terms = np.zeros(job.n)
    with np.errstate(all="ignore"):
        bs = sys.b.reshape(job.nf, 7)
        acc = np.zeros(job.nf)
        for k in range(7):
            acc = acc + xs[:, k] * (lam * xs[:, k] + bs[:, k])
        terms[job.hlist] = acc
    return slot_sum(terms)


def levenberg(est, job, iterations, fn):
    """globalba_ref.levenberg's control flow without the stop flag, from lambda = 1e-16; the trace also
    has edge_chi (per-edge chi2 at the start and of the estimates kept)"""
    tr = SimpleNamespace(iterations=0, rejected=0, lam=[], trials=[], chi_after=[], first_chi=0.0, last_chi=0.0,
                         last_lambda=0.0, margins=[], edge_chi_first=None, edge_chi_last=None, systems=[])
    if job.nf == 0 or len(job.ae) == 0:  # optimize() does nothing without a free active vertex
        return est, tr
    lam = ni = 0.0
    stop_bad = 0
    ok = True
    it = 0
    while it < iterations and ok:
        sys = build_system(est, job, fn)
        cur_chi = sys.chi
        if it == 0:
            lam, ni, stop_bad = LAMBDA_INIT, 2.0, 0
            tr.first_chi = cur_chi
            tr.edge_chi_first = tr.edge_chi_last = sys.chi_e
        tr.systems.append(sys)
        tr.iterations += 1
        tr.lam.append(lam)
        ini_chi = cur_chi
        rho = 0.0
        qmax = 0
        while True:
            x = solve(sys, lam)
            if x is not None:
                trial, xs = step(est, x, job, fn)
                _, chi_e, tmp_chi = active_chi2(trial, job, fn)
                scale = scale_sum(xs, sys, lam, job)
            else:  # a rejected zero step
                tmp_chi, scale = DBL_MAX, 0.0
            scale += 1e-3
            rho = _div(cur_chi - tmp_chi, scale)
            if math.isfinite(tmp_chi) and math.isfinite(cur_chi) and cur_chi != 0:
                tr.margins.append(abs(cur_chi - tmp_chi) / abs(cur_chi))  # rho > 0, rho < 0, rho == 0
            if rho > 0 and math.isfinite(tmp_chi):
                t3 = 2.0 * rho - 1.0
                alpha = min(1.0 - (t3 * t3) * t3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur_chi = tmp_chi
                est = trial
                tr.edge_chi_last = chi_e
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
        tr.last_chi, tr.last_lambda = cur_chi, lam
        it += 1
        if qmax == 10 or rho == 0:
            ok = False
            continue
        if math.isfinite(ini_chi) and ini_chi != 0:
            tr.margins.append(abs((ini_chi - cur_chi) * 1e3 - ini_chi) / abs(ini_chi))  # the stop criterion
        if (ini_chi - cur_chi) * 1e3 < ini_chi:
            stop_bad += 1
        else:
            stop_bad = 0
        if stop_bad >= 3:
            ok = False
    return est, tr


@_ignore
def write_out(est, job):
    """:1144-1199: (Scw (n, 8), Tiw (n, 4, 4) float32, Xw (m, 3) float32)"""
    n = job.n
    R = quat_to_R(est[0:4])
    inv_s = 1.0 / est[7]
    T = np.zeros((n, 4, 4), F32)
    for r in range(3):
        for c in range(3):
            T[:, r, c] = (R[r][c] + np.zeros(n)).astype(F32)
        T[:, r, 3] = (est[4 + r] * inv_s).astype(F32)
    T[:, 3, 3] = 1.0
    X = job.Xw.copy()
    has = job.ref >= 0
    if has.any():
        r = job.ref[has]
        Swc = sim3_inverse(est)
        P = job.Xw[has].astype(np.float64)
        mid = sim3_map(take(job.vScw, r), (P[:, 0], P[:, 1], P[:, 2]))
        out = sim3_map(take(Swc, r), mid)
        X[has] = np.stack(out, 1).astype(F32)
    return as_rows(est), T, X


def optimize_essential_graph(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j,
                             edge_kind, Xw, point_ref, fix_scale, n_iterations, fn=None):
    """Returns a namespace: Scw (n, 8), Tcw (n, 4, 4) float32, Xw (m, 3) float32, iterations, rejected,
    n_free, n_active_edges, first_chi, last_chi, last_lambda, trace, job, fn."""
    fn = fn or Fn()
    job = make_job(Tcw, has_corrected, Scorrected, has_noncorrected, Snoncorrected, fixed, edge_i, edge_j, edge_kind,
                   Xw, point_ref, fix_scale)
    est, tr = levenberg([c.copy() for c in job.vScw], job, int(n_iterations), fn)
    out = SimpleNamespace(trace=tr, job=job, fn=fn, est=est, iterations=tr.iterations, rejected=tr.rejected,
                          n_free=job.nf, n_active_edges=len(job.ae), first_chi=tr.first_chi, last_chi=tr.last_chi,
                          last_lambda=tr.last_lambda)
    out.Scw, out.Tcw, out.Xw = write_out(est, job)
    return out


ARRAYS = ("Tcw", "has_corrected", "Scorrected", "has_noncorrected", "Snoncorrected", "fixed", "edge_i", "edge_j",
          "edge_kind", "Xw", "point_ref")


def run_scene(s, n_iterations, fn=None, edge_perm=None, kf_perm=None):
    """the restatement on an essential_scene dict, optionally with the edges and / or the keyframes
    permuted; the outputs are mapped back to the scene's order"""
    a = {k: np.asarray(s[k]) for k in ARRAYS}
    n = len(a["Tcw"])
    if edge_perm is not None:
        for k in ("edge_i", "edge_j", "edge_kind"):
            a[k] = a[k][edge_perm]
    inv = None
    if kf_perm is not None:  # new index k holds old keyframe kf_perm[k]
        inv = np.empty(n, int)
        inv[kf_perm] = np.arange(n)
        for k in ("Tcw", "has_corrected", "Scorrected", "has_noncorrected", "Snoncorrected", "fixed"):
            a[k] = a[k][kf_perm]
        a["edge_i"], a["edge_j"] = inv[a["edge_i"]], inv[a["edge_j"]]
        a["point_ref"] = np.where(a["point_ref"] >= 0, inv[np.maximum(a["point_ref"], 0)], a["point_ref"])
    r = optimize_essential_graph(*(a[k] for k in ARRAYS), s["fix_scale"], n_iterations, fn)
    if inv is not None:
        r.Scw, r.Tcw = r.Scw[inv], r.Tcw[inv]
    return r


def decisive(r, margin=1e-6):
    """the smallest relative margin over the run's decisions is at least `margin`: every accept / reject,
    rho == 0 and stop-rule decision (trace.margins) and every branch of Sim3(Vector7d) and Sim3::log on
    real updates and perturbed estimates alike (fn.margins)"""
    return min(r.trace.margins + r.fn.margins + [float("inf")]) >= margin
