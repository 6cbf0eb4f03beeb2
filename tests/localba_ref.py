"""CPU restatement of Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:536-885)
from the optimisation on (:759-847; the gather before it and the write-back
after it are the adapter's, include/orbslam2_amd/LocalBundleAdjuster.h) with
the g2o pieces it runs: EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ
(types/types_six_dof_expmap.cpp:112-168, 199-245), BaseBinaryEdge::
constructQuadraticForm (core/base_binary_edge.hpp:43-120), BlockSolver's Schur
complement and back-substitution (core/block_solver.hpp:355-487, 565-610),
OptimizationAlgorithmLevenberg::solve over the whole vector
(core/optimization_algorithm_levenberg.cpp:61-189) and the active set of
SparseOptimizer::initializeOptimization(level 0).  csrc/localba.hip writes the
same expressions in the same association order.

A job: P poses (the n_local local keyframes first, then the fixed ones), M
points, E edges grouped by point.  A pose is free when its fixed flag is clear;
points are all free and marginalised.  Sequential float64 with the float casts
where the reference has them (inputs, the stereo projection's invz, Huber's
delta and dsqr, the written poses and points).  Per-edge terms are numpy
element-wise expressions (one IEEE operation per call); the sums into a pose's
or a point's block run in edge order (np.add.at is sequential), as the kernel's
do; only the robust chi2 sum and computeScale's sum are associated differently
there (the measured bound of tests/test_localba.py covers that).

What is kept: the two rounds (5 iterations with Huber on every edge, then 10
without kernels over the edges not flagged), the double comparison
chi2 > 5.991 | 7.815 || !isDepthPositive(); the active set (a vertex is
optimised, damped and in the lambda maximum only while an unflagged edge touches
it; an edge to a fixed pose contributes to its point only); an active edge's
chi2() is the error of the last trial evaluated, accepted or not, a flagged
edge's is its stale first-round value, and isDepthPositive() reads the kept
estimates; every local pose goes through Converter::toSE3Quat and back.

Deviations: the reduced system is solved by a dense Cholesky without pivoting
in ascending pose order (the reference: Eigen's SimplicialLDLT behind a
fill-reducing ordering), a pivot that is not positive (or NaN) being the failed
solve; the 3x3 inverse is restated from cofactors; a failed solve is a rejected
zero step whose trial is the kept estimate; pbStopFlag is read before the call
only; the products of the quadratic form are associated as written below, Eigen's
order being unknown here.  Parity against a g2o build is unpinned (g2o needs
Eigen).
"""
import math
from types import SimpleNamespace

import numpy as np

import lm_ref
from lm_ref import DBL_MAX, _div, quat_rotate, quat_to_R
from poseopt_ref import (DELTA_MONO, DELTA_STEREO, DSQR_MONO, DSQR_STEREO, se3_exp, se3_from_T, se3_mul,
                         se3_to_T)

F32 = np.float32
TH_MONO, TH_STEREO = 5.991, 7.815  # compared in double (Optimizer.cpp:782, 798)
ITERATIONS = (5, 10)


# ---------------------------------------------------------------- the edges

def edge_errors(Q, Tt, pts, job, float_invz=True):
    """computeError of every edge: (e (E, 3) with e[:, 2] = 0 for a monocular edge, chi2 (E),
    camera-frame point (x, y, z))"""
    pi, li = job.pose_idx, job.point_idx
    q = tuple(Q[pi, k] for k in range(4))
    X = pts[li]
    r = quat_rotate(q, (X[:, 0], X[:, 1], X[:, 2]))
    x, y, z = r[0] + Tt[pi, 0], r[1] + Tt[pi, 1], r[2] + Tt[pi, 2]
    fx, fy, cx, cy, bf = (job.cam[pi, k] for k in range(5))
    stereo, w = job.stereo, job.w
    ou, ov, orr = (job.obs[:, k] for k in range(3))
    with np.errstate(all="ignore"):
        um, vm = (x / z) * fx + cx, (y / z) * fy + cy
        invzf = (1.0 / z).astype(F32).astype(np.float64) if float_invz else 1.0 / z
        us, vs = (x * invzf) * fx + cx, (y * invzf) * fy + cy
        rs = us - bf * invzf
        e0 = ou - np.where(stereo, us, um)
        e1 = ov - np.where(stereo, vs, vm)
        e2 = np.where(stereo, orr - rs, 0.0)
        chi2 = e0 * (w * e0) + e1 * (w * e1)
        chi2 = np.where(stereo, chi2 + e2 * (w * e2), chi2)
    return np.stack([e0, e1, e2], 1), chi2, (x, y, z)


def edge_jacobians(Q, p, job):
    """linearizeOplus: Jl (E, 3, 3) w.r.t. the point, Jp (E, 3, 6) w.r.t. the pose; row 2 is zero
    for a monocular edge"""
    x, y, z = p
    pi = job.pose_idx
    fx, fy, bf = job.cam[pi, 0], job.cam[pi, 1], job.cam[pi, 4]
    stereo = job.stereo
    R = quat_to_R(tuple(Q[pi, k] for k in range(4)))
    E = len(x)
    Jl, Jp = np.zeros((E, 3, 3)), np.zeros((E, 3, 6))
    with np.errstate(all="ignore"):
        z_2 = z * z
        # monocular: -1./z * tmp * R
        s = -1.0 / z
        t00, t01, t02 = s * fx, s * 0.0, s * (((-x) / z) * fx)
        t10, t11, t12 = s * 0.0, s * fy, s * (((-y) / z) * fy)
        for c in range(3):
            m0 = (t00 * R[0][c] + t01 * R[1][c]) + t02 * R[2][c]
            m1 = (t10 * R[0][c] + t11 * R[1][c]) + t12 * R[2][c]
            # stereo: entry by entry
            s0 = ((-fx) * R[0][c]) / z + ((fx * x) * R[2][c]) / z_2
            s1 = ((-fy) * R[1][c]) / z + ((fy * y) * R[2][c]) / z_2
            Jl[:, 0, c] = np.where(stereo, s0, m0)
            Jl[:, 1, c] = np.where(stereo, s1, m1)
            Jl[:, 2, c] = np.where(stereo, s0 - (bf * R[2][c]) / z_2, 0.0)
        Jp[:, 0, 0] = ((x * y) / z_2) * fx
        Jp[:, 0, 1] = (-(1.0 + (x * x) / z_2)) * fx
        Jp[:, 0, 2] = (y / z) * fx
        Jp[:, 0, 3] = (-1.0 / z) * fx
        Jp[:, 0, 5] = (x / z_2) * fx
        Jp[:, 1, 0] = (1.0 + (y * y) / z_2) * fy
        Jp[:, 1, 1] = (((-x) * y) / z_2) * fy
        Jp[:, 1, 2] = ((-x) / z) * fy
        Jp[:, 1, 4] = (-1.0 / z) * fy
        Jp[:, 1, 5] = (y / z_2) * fy
        Jp[:, 2, 0] = np.where(stereo, Jp[:, 0, 0] - (bf * y) / z_2, 0.0)
        Jp[:, 2, 1] = np.where(stereo, Jp[:, 0, 1] + (bf * x) / z_2, 0.0)
        Jp[:, 2, 2] = np.where(stereo, Jp[:, 0, 2], 0.0)
        Jp[:, 2, 3] = np.where(stereo, Jp[:, 0, 3], 0.0)
        Jp[:, 2, 5] = np.where(stereo, Jp[:, 0, 5] - bf / z_2, 0.0)
    return Jl, Jp


def _rows3(A, B):
    """sum over the three residual rows of A[:, r, :, None] * B[:, r, None, :], left to right"""
    return (A[:, 0, :, None] * B[:, 0, None, :] + A[:, 1, :, None] * B[:, 1, None, :]) + A[:, 2, :, None] * B[:, 2, None, :]


# ---------------------------------------------------------------- structure of one optimisation

def structure(job, level1):
    """the active set of initializeOptimization(0) and the index lists of the Schur complement"""
    P, M = job.P, job.M
    act = ~level1
    pi, li = job.pose_idx, job.point_idx
    pose_touched = np.zeros(P, bool)
    pose_touched[pi[act]] = True
    point_active = np.zeros(M, bool)
    point_active[li[act]] = True
    pose_free = pose_touched & ~job.fixed
    hidx = np.full(P, -1)
    hidx[pose_free] = np.arange(int(pose_free.sum()))
    lidx = np.full(M, -1)
    lidx[point_active] = np.arange(int(point_active.sum()))
    ea = np.nonzero(act)[0]                        # active edges, ascending
    ef = ea[pose_free[pi[ea]]]                     # active edges with a free pose: those have a B block
    # pairs (e, e2): for each free pose a ascending, its edges e ascending, the edges e2 of e's point
    # ascending whose pose b is free with hidx[b] >= hidx[a]
    by_point = {}
    for e in ef:
        by_point.setdefault(int(li[e]), []).append(int(e))
    pe, pe2 = [], []
    for a in np.nonzero(pose_free)[0]:
        for e in ef[pi[ef] == a]:
            for e2 in by_point[int(li[e])]:
                if hidx[pi[e2]] >= hidx[a]:
                    pe.append(int(e))
                    pe2.append(e2)
    return SimpleNamespace(act=act, ea=ea, ef=ef, pose_free=pose_free, point_active=point_active, hidx=hidx,
                           lidx=lidx, nf=int(pose_free.sum()), nl=int(point_active.sum()),
                           pe=np.asarray(pe, int), pe2=np.asarray(pe2, int))


def build_system(est, job, st, robust, last_chi2):
    """computeActiveErrors + activeRobustChi2 + buildSystem at `est`"""
    Q, Tt, pts = est
    e, chi2, p = edge_errors(Q, Tt, pts, job)
    last_chi2[st.act] = chi2[st.act]
    Jl, Jp = edge_jacobians(Q, p, job)
    if robust:
        rho0, rho1 = lm_ref.huber(chi2, job.delta, job.dsqr)
    else:
        rho0, rho1 = chi2, np.ones_like(chi2)
    P, M = job.P, job.M
    with np.errstate(all="ignore"):
        Wt = rho1 * job.w
        omr = rho1[:, None] * (-(job.w[:, None] * e))
        WJp, WJl = Wt[:, None, None] * Jp, Wt[:, None, None] * Jl
        Hpp, bp = np.zeros((P, 6, 6)), np.zeros((P, 6))
        Hll, bl = np.zeros((M, 3, 3)), np.zeros((M, 3))
        ea, ef = st.ea, st.ef
        np.add.at(Hll, job.point_idx[ea], _rows3(WJl[ea], Jl[ea]))
        np.add.at(bl, job.point_idx[ea],
                  (Jl[ea, 0, :] * omr[ea, 0, None] + Jl[ea, 1, :] * omr[ea, 1, None]) + Jl[ea, 2, :] * omr[ea, 2, None])
        np.add.at(Hpp, job.pose_idx[ef], _rows3(WJp[ef], Jp[ef]))
        np.add.at(bp, job.pose_idx[ef],
                  (Jp[ef, 0, :] * omr[ef, 0, None] + Jp[ef, 1, :] * omr[ef, 1, None]) + Jp[ef, 2, :] * omr[ef, 2, None])
        B = _rows3(WJp, Jl)  # (E, 6, 3): the pose-point block of an edge
        chi = float(np.sum(rho0[ea]))
    return SimpleNamespace(Hpp=Hpp, bp=bp, Hll=Hll, bl=bl, B=B, chi=chi)


def trial_chi(trial, job, st, robust, last_chi2):
    Q, Tt, pts = trial
    _, chi2, _ = edge_errors(Q, Tt, pts, job)
    last_chi2[st.act] = chi2[st.act]
    rho0 = lm_ref.huber(chi2, job.delta, job.dsqr)[0] if robust else chi2
    with np.errstate(all="ignore"):
        return float(np.sum(rho0[st.ea]))


def point_inverses(Hll, lam):
    """(Hll + lam I)^-1 of every point from cofactors: (M, 3, 3), symmetric"""
    with np.errstate(all="ignore"):
        a, b, c = Hll[:, 0, 0] + lam, Hll[:, 0, 1], Hll[:, 0, 2]
        d, e, f = Hll[:, 1, 1] + lam, Hll[:, 1, 2], Hll[:, 2, 2] + lam
        c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
        c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
        inv = 1.0 / ((a * c00 + b * c01) + c * c02)
        D = np.empty_like(Hll)
        D[:, 0, 0], D[:, 0, 1], D[:, 0, 2] = c00 * inv, c01 * inv, c02 * inv
        D[:, 1, 0], D[:, 1, 1], D[:, 1, 2] = D[:, 0, 1], c11 * inv, c12 * inv
        D[:, 2, 0], D[:, 2, 1], D[:, 2, 2] = D[:, 0, 2], D[:, 1, 2], c22 * inv
    return D


def _mat3_vec(D, v):
    return np.stack([(D[:, c, 0] * v[:, 0] + D[:, c, 1] * v[:, 1]) + D[:, c, 2] * v[:, 2] for c in range(3)], 1)


def schur_system(sys, job, st, lam):
    """the reduced system of BlockSolver::solve: (S (n, n) symmetric, b_schur (n), Dinv)"""
    pi, li = job.pose_idx, job.point_idx
    nf = st.nf
    free = np.nonzero(st.pose_free)[0]
    with np.errstate(all="ignore"):
        Dinv = point_inverses(sys.Hll, lam)
        v = _mat3_vec(Dinv, sys.bl)
        ef = st.ef
        B = sys.B
        coef = np.zeros((nf, 6))
        ve = v[li[ef]]
        np.add.at(coef, st.hidx[pi[ef]],
                  (B[ef, :, 0] * ve[:, 0, None] + B[ef, :, 1] * ve[:, 1, None]) + B[ef, :, 2] * ve[:, 2, None])
        De = Dinv[li]
        BD = (B[:, :, 0, None] * De[:, None, 0, :] + B[:, :, 1, None] * De[:, None, 1, :]) + B[:, :, 2, None] * De[:, None, 2, :]
        S4 = np.zeros((nf, nf, 6, 6))
        for i, p in enumerate(free):
            S4[i, i] = sys.Hpp[p]
            for j in range(6):
                S4[i, i, j, j] = sys.Hpp[p, j, j] + lam
        pe, pe2 = st.pe, st.pe2
        if len(pe):
            X, Y = BD[pe], B[pe2]
            contrib = (X[:, :, None, 0] * Y[:, None, :, 0] + X[:, :, None, 1] * Y[:, None, :, 1]) + X[:, :, None, 2] * Y[:, None, :, 2]
            np.subtract.at(S4, (st.hidx[pi[pe]], st.hidx[pi[pe2]]), contrib)
        n = 6 * nf
        S = np.zeros((n, n))
        for i in range(nf):
            for j in range(i, nf):
                S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = S4[i, j]
        S = np.triu(S) + np.triu(S, 1).T
        bs = sys.bp[free] - coef
    return S, bs.reshape(-1), Dinv


def schur_solve(sys, job, st, lam):
    """BlockSolver::solve at lambda: (x_p (nf, 6), x_l (M, 3) with zeros at inactive points), or
    None when the pose solve fails"""
    pi, li = job.pose_idx, job.point_idx
    S, bs, Dinv = schur_system(sys, job, st, lam)
    if st.nf:
        xp = lm_ref.cholesky_solve(S, bs, 0.0)
        if xp is None:
            return None
        xp = np.asarray(xp).reshape(st.nf, 6)
    else:
        xp = np.zeros((0, 6))
    with np.errstate(all="ignore"):
        t = sys.bl.copy()
        ef = st.ef
        if len(ef):
            xe = xp[st.hidx[pi[ef]]]
            B = sys.B[ef]
            dot = B[:, 0, :] * xe[:, 0, None]
            for a in range(1, 6):
                dot = dot + B[:, a, :] * xe[:, a, None]
            np.subtract.at(t, li[ef], dot)
        xl = _mat3_vec(Dinv, t)
    xl[~st.point_active] = 0.0
    return xp, xl


def oplus(est, xp, xl, st):
    Q, Tt, pts = (a.copy() for a in est)
    for p in np.nonzero(st.pose_free)[0]:
        q, t = se3_mul(se3_exp([float(v) for v in xp[st.hidx[p]]]), (list(Q[p]), list(Tt[p])))
        Q[p], Tt[p] = q, t
    with np.errstate(all="ignore"):
        pts[st.point_active] = pts[st.point_active] + xl[st.point_active]
    return Q, Tt, pts


def levenberg(est, job, st, iterations, robust, last_chi2):
    """lm_ref.levenberg's control flow over the whole vector, the solve being the Schur solve"""
    tr = SimpleNamespace(iterations=0, rejected=0, lam=[], trials=[], chi_after=[])
    if st.nf + st.nl == 0:  # optimize() returns at once without an active vertex
        return est, tr
    free = np.nonzero(st.pose_free)[0]
    pts_a = np.nonzero(st.point_active)[0]
    lam = ni = 0.0
    stop_bad = 0
    for it in range(iterations):
        sys = build_system(est, job, st, robust, last_chi2)
        cur_chi = sys.chi
        if it == 0:
            max_diag = 0.0
            for H, idx, d in ((sys.Hpp, free, 6), (sys.Hll, pts_a, 3)):
                for i in idx:
                    for j in range(d):
                        a = abs(float(H[i, j, j]))
                        max_diag = max_diag if a < max_diag else a
            lam = 1e-5 * max_diag
            ni = 2.0
            stop_bad = 0
        tr.iterations += 1
        tr.lam.append(lam)
        ini_chi = cur_chi
        rho = 0.0
        qmax = 0
        b_all = [float(v) for p in free for v in sys.bp[p]] + [float(v) for m in pts_a for v in sys.bl[m]]
        while True:
            sol = schur_solve(sys, job, st, lam)
            if sol is not None:
                xp, xl = sol
                trial = oplus(est, xp, xl, st)
                tmp_chi = trial_chi(trial, job, st, robust, last_chi2)
                x_all = [float(v) for v in xp.reshape(-1)] + [float(v) for m in pts_a for v in xl[m]]
            else:  # a rejected zero step; the errors are those of the kept estimate
                trial_chi(est, job, st, robust, last_chi2)
                x_all = [0.0] * len(b_all)
                tmp_chi = DBL_MAX
            scale = 0.0
            for xj, bj in zip(x_all, b_all):
                scale += xj * (lam * xj + bj)
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
    return est, tr


# ---------------------------------------------------------------- Optimizer::LocalBundleAdjustment

def make_job(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local):
    """the inputs as float32, widened"""
    Tcw = np.asarray(Tcw, F32)
    Tcw = Tcw.reshape(len(Tcw), -1, 4)[:, :3]  # (P, 4, 4), (P, 3, 4) or flat rows of either
    obs = np.asarray(obs, F32).reshape(-1, 3).astype(np.float64)
    stereo = obs[:, 2] >= 0
    P = len(Tcw)
    fixed = np.asarray(fixed).astype(bool).copy()
    fixed[n_local:] = True
    return SimpleNamespace(
        P=P, M=len(np.asarray(Xw).reshape(-1, 3)), E=len(obs), n_local=int(n_local), Tcw=Tcw, fixed=fixed,
        cam=np.asarray(cam, F32).reshape(-1, 5).astype(np.float64), Xw=np.asarray(Xw, F32).reshape(-1, 3),
        pose_idx=np.asarray(pose_idx, int).reshape(-1), point_idx=np.asarray(point_idx, int).reshape(-1), obs=obs,
        w=np.asarray(inv_sigma2, F32).reshape(-1).astype(np.float64), stereo=stereo,
        delta=np.where(stereo, DELTA_STEREO, DELTA_MONO), dsqr=np.where(stereo, DSQR_STEREO, DSQR_MONO),
        thr=np.where(stereo, TH_STEREO, TH_MONO))


def local_bundle_adjustment(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local):
    """Returns a namespace: Tcw (n_local, 4, 4) float32, Xw (M, 3) float32, erase (E bool),
    flag_first (E bool), n_bad_first, n_erase, rounds, trace (per round), what the two checks read:
    chi2_first, z_first, chi2_final, z_final (E float64), and the estimates (q (P, 4), t (P, 3),
    points (M, 3) in float64) after the first round and at the end: est_first, est."""
    job = make_job(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local)
    P, M, E = job.P, job.M, job.E
    Q, Tt = np.zeros((P, 4)), np.zeros((P, 3))
    for p in range(P):
        Q[p], Tt[p] = se3_from_T(job.Tcw[p])
    est = (Q, Tt, job.Xw.astype(np.float64))
    out = SimpleNamespace(rounds=0, trace=[], erase=np.zeros(E, bool), flag_first=np.zeros(E, bool), n_bad_first=0,
                          n_erase=0, chi2_first=np.zeros(E), z_first=np.ones(E), chi2_final=np.zeros(E),
                          z_final=np.ones(E), job=job)
    if E:
        last_chi2 = np.zeros(E)
        level1 = np.zeros(E, bool)
        for rnd in range(2):
            st = structure(job, level1)
            est, tr = levenberg(est, job, st, ITERATIONS[rnd], rnd == 0, last_chi2)
            out.trace.append(tr)
            z = edge_errors(*est, job)[2][2]
            with np.errstate(all="ignore"):
                flag = (last_chi2 > job.thr) | ~(z > 0.0)
            if rnd == 0:
                level1 = flag
                out.flag_first, out.n_bad_first = flag, int(flag.sum())
                out.chi2_first, out.z_first = last_chi2.copy(), z
                out.est_first = tuple(a.copy() for a in est)
            else:
                out.erase, out.n_erase = flag, int(flag.sum())
                out.chi2_final, out.z_final = last_chi2.copy(), z
        out.rounds = 2
    out.est = est
    out.Tcw = np.stack([se3_to_T((list(est[0][p]), list(est[1][p]))) for p in range(job.n_local)]) \
        if job.n_local else np.zeros((0, 4, 4), F32)
    out.Xw = est[2].astype(F32)
    return out


def run_scene(s, point_perm=None, edge_perm_seed=None):
    """the restatement on a synth.localba_scene dict, optionally with the points permuted and the
    edges permuted within each point; results are mapped back to the scene's order"""
    M, E = len(s["Xw"]), len(s["obs"])
    pperm = np.arange(M) if point_perm is None else np.asarray(point_perm)
    inv = np.empty(M, int)
    inv[pperm] = np.arange(M)  # new index of old point m
    new_pt = inv[s["point_idx"]]
    key = np.zeros(E) if edge_perm_seed is None else np.random.default_rng(edge_perm_seed).uniform(size=E)
    order = np.lexsort((key, new_pt)) if edge_perm_seed is not None else np.argsort(new_pt, kind="stable")
    r = local_bundle_adjustment(s["Tcw"], s["fixed"], s["cam"], s["Xw"][pperm], s["pose_idx"][order], new_pt[order],
                                s["obs"][order], s["inv_sigma2"][order], s["n_local"])
    back = np.empty(E, int)
    back[order] = np.arange(E)
    for name in ("erase", "flag_first", "chi2_first", "z_first", "chi2_final", "z_final"):
        setattr(r, name, getattr(r, name)[back])
    r.Xw = r.Xw[inv]
    r.est = (r.est[0], r.est[1], r.est[2][inv])
    if r.rounds:
        r.est_first = (r.est_first[0], r.est_first[1], r.est_first[2][inv])
    return r


def margins(r, obs):
    """smallest relative distance from its threshold of a chi2 that either check read, and the
    smallest |z| either check read, of a run_scene result (scene order)"""
    if r.rounds == 0:
        return float("inf"), float("inf")
    thr = np.where(np.asarray(obs, F32).reshape(-1, 3)[:, 2] >= 0, TH_STEREO, TH_MONO)
    m = min(float(np.min(np.abs(c - thr) / thr)) for c in (r.chi2_first, r.chi2_final))
    return m, min(float(np.min(np.abs(z))) for z in (r.z_first, r.z_final))
