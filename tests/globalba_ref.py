"""CPU restatement of Optimizer::BundleAdjustment / GlobalBundleAdjustemnt
(src/Optimizer.cpp:72-269) from the optimisation on (the gather and the
write-back are the adapter's, include/orbslam2_amd/BundleAdjuster.h), with
SparseOptimizer::optimize's loop and its two polls of the force-stop flag
(core/sparse_optimizer.cpp:354-419, core/optimization_algorithm_levenberg.cpp:149).
csrc/globalba.hip writes the same expressions in the same association order.

Everything per edge, per vertex and of the Schur complement is localba_ref's
(make_job, structure, build_system, trial_chi, schur_system, oplus), with the
monocular Huber delta (float)sqrt(5.99) of :112 in place of LocalBA's 5.991.
What differs from localba_ref:

* one optimize(n_iterations): no second round, no classification, every edge at
  level 0, Huber on every edge iff `robust`;
* every pose is an output pose, and `fixed` is honoured for every pose;
* the reduced system is solved by blocked_order_solve: factor and forward
  substitution in lm_ref.cholesky_solve's order (every entry's subtractions in
  ascending k, which a right-looking blocked factorisation keeps for any panel
  width), the back-substitution column by column from the last: x[i] = s[i] /
  L[i][i], then s[k] -= L[i][k] x[i] for every k < i.  An entry of s is updated
  in descending i, where cholesky_solve's row form subtracts in ascending k;
* the stop flag: `stop_at` = k makes the k-th poll (counted from 0 over both
  kinds, in the order g2o makes them) see the flag set.  g2o polls at the top
  of every iteration that i < iterations admits, and after a rejected trial
  that would be followed by another (rho < 0 and qmax < 10).

Deviations, as localba_ref states its own: dense Cholesky without pivoting in
ascending pose order in place of Eigen's sparse solver; a pivot that is not
positive (or NaN) is the failed solve; a failed solve is a rejected zero step;
the products are associated as written; parity against a g2o build is unpinned.
"""
import math
from types import SimpleNamespace

import numpy as np

import lm_ref
import localba_ref
from lm_ref import DBL_MAX, _div
from poseopt_ref import DELTA_STEREO, DSQR_STEREO, se3_from_T, se3_to_T

F32 = np.float32
DELTA_MONO = float(F32(math.sqrt(5.99)))  # Optimizer.cpp:112
DSQR_MONO = float(F32(DELTA_MONO * DELTA_MONO))


def blocked_order_solve(S, b):
    """S x = b by Cholesky in the order of csrc/globalba.hip: (x, L, y), or None when a pivot is not
    positive (or NaN).  L and y are bit-equal to lm_ref.cholesky_solve's; x is not (see above).
    The k loops are sequential, the rows vectorised."""
    n = len(b)
    A = np.array(S, np.float64).reshape(n, n)
    M = np.zeros((n + 1, n))  # the lower triangle, and b as one more row
    M[:n] = np.tril(A)
    M[n] = np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        for j in range(n):
            r = M[j:, j].copy()
            for k in range(j):
                r -= M[j:, k] * M[j, k]
            if not r[0] > 0:
                return None
            d = math.sqrt(r[0])
            M[j, j] = d
            M[j + 1:, j] = r[1:] / d
        L, y = M[:n].copy(), M[n].copy()
        s, x = y.copy(), np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = s[i] / L[i, i]
            s[:i] -= L[i, :i] * x[i]
    return x, L, y


def schur_solve(sys, job, st, lam):
    """localba_ref.schur_solve with the reduced system solved by blocked_order_solve"""
    pi, li = job.pose_idx, job.point_idx
    S, bs, Dinv = localba_ref.schur_system(sys, job, st, lam)
    if st.nf:
        sol = blocked_order_solve(S, bs)
        if sol is None:
            return None
        xp = sol[0].reshape(st.nf, 6)
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
        xl = localba_ref._mat3_vec(Dinv, t)
    xl[~st.point_active] = 0.0
    return xp, xl


def levenberg(est, job, st, iterations, robust, stop_at=None):
    """localba_ref.levenberg's control flow inside SparseOptimizer::optimize's loop, with the two
    polls.  Returns (estimates, trace); the trace also has stopped, iterations_applied, first_chi,
    last_chi, margins (the relative distance of every chi2 decision from its threshold)."""
    tr = SimpleNamespace(iterations=0, rejected=0, lam=[], trials=[], chi_after=[], stopped=0, iterations_applied=0,
                         first_chi=0.0, last_chi=0.0, last_lambda=0.0, margins=[], polls=0)
    if st.nf + st.nl == 0:  # optimize() returns at once without an active vertex
        return est, tr
    polls = [0]

    def terminate():
        polls[0] += 1
        tr.polls = polls[0]
        return stop_at is not None and polls[0] - 1 >= stop_at

    free = np.nonzero(st.pose_free)[0]
    pts_a = np.nonzero(st.point_active)[0]
    last_chi2 = np.zeros(job.E)
    lam = ni = 0.0
    stop_bad = 0
    ok = True
    it = 0
    while it < iterations:
        if terminate():
            tr.stopped = 1
            break
        if not ok:
            break
        sys = localba_ref.build_system(est, job, st, robust, last_chi2)
        cur_chi = sys.chi
        if it == 0:
            max_diag = 0.0
            with np.errstate(all="ignore"):
                for H, idx, d in ((sys.Hpp, free, 6), (sys.Hll, pts_a, 3)):
                    if len(idx):
                        diag = np.abs(H[idx][:, np.arange(d), np.arange(d)])
                        m = float(np.nan) if np.isnan(diag).any() else float(diag.max())
                        max_diag = m if not m < max_diag else max_diag  # a NaN wins: the kernel's integer maximum
            lam = 1e-5 * max_diag
            ni = 2.0
            stop_bad = 0
            tr.first_chi = cur_chi
        tr.iterations += 1
        tr.lam.append(lam)
        ini_chi = cur_chi
        rho = 0.0
        qmax = 0
        b_all = np.concatenate([sys.bp[free].reshape(-1), sys.bl[pts_a].reshape(-1)])
        stopped_here = False
        while True:
            sol = schur_solve(sys, job, st, lam)
            if sol is not None:
                xp, xl = sol
                trial = localba_ref.oplus(est, xp, xl, st)
                tmp_chi = localba_ref.trial_chi(trial, job, st, robust, last_chi2)
                x_all = np.concatenate([xp.reshape(-1), xl[pts_a].reshape(-1)])
            else:  # a rejected zero step
                x_all = np.zeros(len(b_all))
                tmp_chi = DBL_MAX
            scale = 0.0
            with np.errstate(all="ignore"):
                for term in x_all * (lam * x_all + b_all):
                    scale += float(term)
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
            if terminate():
                stopped_here = True
                break
        tr.last_chi, tr.last_lambda = cur_chi, lam
        it += 1
        if stopped_here:
            tr.stopped = 2
            break
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
    tr.iterations_applied = tr.iterations - 1 if tr.stopped == 2 else tr.iterations
    return est, tr


def make_job(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2):
    """localba_ref.make_job with every pose an output pose and the deltas of :112-113"""
    job = localba_ref.make_job(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, len(Tcw))
    job.delta = np.where(job.stereo, DELTA_STEREO, DELTA_MONO)
    job.dsqr = np.where(job.stereo, DSQR_STEREO, DSQR_MONO)
    return job


def bundle_adjustment(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_iterations, robust, stop_at=None,
                      job_hook=None):
    """Returns a namespace: Tcw (P, 4, 4) float32, Xw (M, 3) float32, iterations, rejected, stopped,
    iterations_applied, n_free, n_active_points, first_chi, last_chi, last_lambda, trace, est.
    job_hook(job) may change the job before it runs (the tests swap delta / dsqr)."""
    job = make_job(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2)
    if job_hook is not None:
        job_hook(job)
    P = job.P
    Q, Tt = np.zeros((P, 4)), np.zeros((P, 3))
    for p in range(P):
        Q[p], Tt[p] = se3_from_T(job.Tcw[p])
    est = (Q, Tt, job.Xw.astype(np.float64))
    st = localba_ref.structure(job, np.zeros(job.E, bool))
    est, tr = levenberg(est, job, st, int(n_iterations), bool(robust), stop_at)
    out = SimpleNamespace(trace=tr, job=job, est=est, iterations=tr.iterations, rejected=tr.rejected, stopped=tr.stopped,
                          iterations_applied=tr.iterations_applied, n_free=st.nf, n_active_points=st.nl,
                          first_chi=tr.first_chi, last_chi=tr.last_chi, last_lambda=tr.last_lambda)
    out.Tcw = np.stack([se3_to_T((list(est[0][p]), list(est[1][p]))) for p in range(P)]).astype(F32) if P else \
        np.zeros((0, 4, 4), F32)
    out.Xw = est[2].astype(F32)
    return out


def run_scene(s, n_iterations, robust, stop_at=None, point_perm=None, edge_perm_seed=None, job_hook=None):
    """the restatement on a synth.localba_scene dict, optionally with the points permuted and the
    edges permuted within each point; the points are mapped back to the scene's order"""
    M, E = len(s["Xw"]), len(s["obs"])
    pperm = np.arange(M) if point_perm is None else np.asarray(point_perm)
    inv = np.empty(M, int)
    inv[pperm] = np.arange(M)
    new_pt = inv[s["point_idx"]] if E else np.zeros(0, int)
    key = np.zeros(E) if edge_perm_seed is None else np.random.default_rng(edge_perm_seed).uniform(size=E)
    order = np.lexsort((key, new_pt)) if edge_perm_seed is not None else np.argsort(new_pt, kind="stable")
    r = bundle_adjustment(s["Tcw"], s["fixed"], s["cam"], s["Xw"][pperm], s["pose_idx"][order], new_pt[order],
                          s["obs"][order], s["inv_sigma2"][order], n_iterations, robust, stop_at, job_hook)
    r.Xw = r.Xw[inv]
    r.est = (r.est[0], r.est[1], r.est[2][inv])
    return r


def decisive(r, margin=1e-6):
    """every chi2 decision of the run (accept / reject, rho == 0, the stop criterion) stayed `margin`
    (relative) from its threshold: the integer outcomes are then the kernel's too"""
    return all(m >= margin for m in r.trace.margins)
