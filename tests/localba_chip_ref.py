"""CPU restatement of Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:536-885)
as csrc/localba_chip.hip runs it (include/orbgpu_localba_chip.h): localba_ref's
two rounds on globalba_ref's solver, with g2o's polls of the force-stop flag.

It is localba_ref.local_bundle_adjustment with three changes:

* the Schur solve is globalba_ref.schur_solve: blocked_order_solve with the
  column-oriented back-substitution;
* computeLambdaInit's maximum follows globalba_ref: a NaN wins wherever it
  stands;
* levenberg has globalba_ref.levenberg's two polls, over the caller's last_chi2
  array, and the counter of polls is shared by both rounds.  Polls are counted
  from 0: the first round's (the top of every iteration that i < iterations
  admits, and after a rejected trial that another would follow), the read
  between the rounds (Optimizer.cpp:764), the second round's.  `stop_at` = k
  makes poll k and every later one see the flag.

Everything else is localba_ref's: structure(job, level1) per round, Huber in the
first round only, the double comparison chi2 > 5.991 | 7.815 || !(z > 0) with z
from the kept estimates and chi2 that of the last trial evaluated, a level-1
edge's stale value, the chi2 pass on the kept estimates after a failed solve,
the round trip of every local pose, lambda, ni and the stop counter afresh in
the second round.

Stop rules: a poll inside a round ends that round (stopped = 1 at the top of an
iteration, 2 after a rejected trial).  When the read between the rounds sees
the flag, rounds = 1: nothing goes to level 1, there is no second round and the
final test runs over all edges; when it does not, the second round runs even
after a stopped first one.  An edge never evaluated has chi2 0.

Deviations: localba_ref's and globalba_ref's; parity against a g2o build is
unpinned.
"""
import math
from types import SimpleNamespace

import numpy as np

import globalba_ref
import localba_ref
from lm_ref import DBL_MAX, _div
from poseopt_ref import se3_from_T, se3_to_T

F32 = np.float32
ITERATIONS = localba_ref.ITERATIONS
TOP, REJECTED, BETWEEN = "top", "rejected", "between"  # the kinds of poll


class Polls:
    """the shared counter: kinds[k] is what poll k was, stop_poll the first that saw the flag"""

    def __init__(self, stop_at=None):
        self.stop_at, self.kinds, self.stop_poll = stop_at, [], -1

    def __call__(self, kind):
        k = len(self.kinds)
        self.kinds.append(kind)
        seen = self.stop_at is not None and k >= self.stop_at
        if seen and self.stop_poll < 0:
            self.stop_poll = k
        return seen


def levenberg(est, job, st, iterations, robust, last_chi2, terminate):
    """globalba_ref.levenberg over the caller's last_chi2 and poll counter; after a failed solve the
    edges get the errors of the kept estimate (localba_ref)"""
    tr = SimpleNamespace(iterations=0, rejected=0, lam=[], trials=[], chi_after=[], stopped=0, iterations_applied=0,
                         margins=[])
    if st.nf + st.nl == 0:  # optimize() returns at once without an active vertex
        return est, tr
    free = np.nonzero(st.pose_free)[0]
    pts_a = np.nonzero(st.point_active)[0]
    lam = ni = 0.0
    stop_bad = 0
    ok = True
    it = 0
    while it < iterations:
        if terminate(TOP):
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
                        max_diag = m if not m < max_diag else max_diag  # a NaN wins
            lam = 1e-5 * max_diag
            ni = 2.0
            stop_bad = 0
        tr.iterations += 1
        tr.lam.append(lam)
        ini_chi = cur_chi
        rho = 0.0
        qmax = 0
        b_all = np.concatenate([sys.bp[free].reshape(-1), sys.bl[pts_a].reshape(-1)])
        stopped_here = False
        while True:
            sol = globalba_ref.schur_solve(sys, job, st, lam)
            if sol is not None:
                xp, xl = sol
                trial = localba_ref.oplus(est, xp, xl, st)
                tmp_chi = localba_ref.trial_chi(trial, job, st, robust, last_chi2)
                x_all = np.concatenate([xp.reshape(-1), xl[pts_a].reshape(-1)])
            else:  # a rejected zero step; the errors are those of the kept estimate
                localba_ref.trial_chi(est, job, st, robust, last_chi2)
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
            if terminate(REJECTED):
                stopped_here = True
                break
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


def local_bundle_adjustment(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local, iterations=ITERATIONS,
                            stop_at=None):
    """Returns localba_ref.local_bundle_adjustment's namespace (chi2_first / z_first are what the
    classification read, chi2_final / z_final what the final test read) and, as the C ABI's result has
    them: rounds, n_bad_first, n_erase, stop_poll, polls, and per round lm_iterations, lm_rejected,
    stopped, iterations_applied, n_free, n_active_points; poll_kinds[k] is the kind of poll k."""
    job = localba_ref.make_job(Tcw, fixed, cam, Xw, pose_idx, point_idx, obs, inv_sigma2, n_local)
    P, E = job.P, job.E
    Q, Tt = np.zeros((P, 4)), np.zeros((P, 3))
    for p in range(P):
        Q[p], Tt[p] = se3_from_T(job.Tcw[p])
    est = (Q, Tt, job.Xw.astype(np.float64))
    poll = Polls(stop_at)
    out = SimpleNamespace(rounds=0, trace=[], erase=np.zeros(E, bool), flag_first=np.zeros(E, bool), n_bad_first=0,
                          n_erase=0, chi2_first=None, z_first=None, chi2_final=np.zeros(E), z_final=np.ones(E), job=job,
                          lm_iterations=[0, 0], lm_rejected=[0, 0], stopped=[0, 0], iterations_applied=[0, 0],
                          n_free=[0, 0], n_active_points=[0, 0])

    def test(last_chi2):
        z = localba_ref.edge_errors(*est, job)[2][2]
        with np.errstate(all="ignore"):
            return (last_chi2 > job.thr) | ~(z > 0.0), z

    def optimize(rnd, level1, last_chi2):
        st = localba_ref.structure(job, level1)
        e, tr = levenberg(est, job, st, int(iterations[rnd]), rnd == 0, last_chi2, poll)
        out.trace.append(tr)
        out.lm_iterations[rnd], out.lm_rejected[rnd], out.stopped[rnd] = tr.iterations, tr.rejected, tr.stopped
        out.iterations_applied[rnd], out.n_free[rnd], out.n_active_points[rnd] = tr.iterations_applied, st.nf, st.nl
        return e

    if E:
        last_chi2 = np.zeros(E)  # an edge never evaluated has chi2 0
        est = optimize(0, np.zeros(E, bool), last_chi2)
        out.rounds = 1
        out.est_first = tuple(a.copy() for a in est)
        if not poll(BETWEEN):  # Optimizer.cpp:764-766
            flag, z = test(last_chi2)
            out.flag_first, out.n_bad_first = flag, int(flag.sum())
            out.chi2_first, out.z_first = last_chi2.copy(), z
            est = optimize(1, flag, last_chi2)
            out.rounds = 2
        flag, z = test(last_chi2)
        out.erase, out.n_erase = flag, int(flag.sum())
        out.chi2_final, out.z_final = last_chi2.copy(), z
    out.polls, out.poll_kinds, out.stop_poll = len(poll.kinds), list(poll.kinds), poll.stop_poll
    out.est = est
    out.Tcw = np.stack([se3_to_T((list(est[0][p]), list(est[1][p]))) for p in range(job.n_local)]).astype(F32) \
        if job.n_local else np.zeros((0, 4, 4), F32)
    out.Xw = est[2].astype(F32)
    return out


def run_scene(s, iterations=ITERATIONS, stop_at=None, point_perm=None, edge_perm_seed=None):
    """the restatement on a synth.localba_scene dict, optionally with the points permuted and the
    edges permuted within each point; results are mapped back to the scene's order"""
    M, E = len(s["Xw"]), len(s["obs"])
    pperm = np.arange(M) if point_perm is None else np.asarray(point_perm)
    inv = np.empty(M, int)
    inv[pperm] = np.arange(M)  # new index of old point m
    new_pt = inv[s["point_idx"]] if E else np.zeros(0, int)
    key = np.zeros(E) if edge_perm_seed is None else np.random.default_rng(edge_perm_seed).uniform(size=E)
    order = np.lexsort((key, new_pt)) if edge_perm_seed is not None else np.argsort(new_pt, kind="stable")
    r = local_bundle_adjustment(s["Tcw"], s["fixed"], s["cam"], s["Xw"][pperm], s["pose_idx"][order], new_pt[order],
                                s["obs"][order], s["inv_sigma2"][order], s["n_local"], iterations, stop_at)
    back = np.empty(E, int)
    back[order] = np.arange(E)
    for name in ("erase", "flag_first", "chi2_first", "z_first", "chi2_final", "z_final"):
        if getattr(r, name) is not None:
            setattr(r, name, getattr(r, name)[back])
    r.Xw = r.Xw[inv]
    r.est = (r.est[0], r.est[1], r.est[2][inv])
    return r


def margins(r, obs):
    """smallest relative distance from its threshold of a chi2 that either check read, and the smallest
    |z| either check read, of a run_scene result (scene order)"""
    if r.rounds == 0:
        return float("inf"), float("inf")
    thr = np.where(np.asarray(obs, F32).reshape(-1, 3)[:, 2] >= 0, localba_ref.TH_STEREO, localba_ref.TH_MONO)
    read = [(r.chi2_final, r.z_final)] + ([(r.chi2_first, r.z_first)] if r.chi2_first is not None else [])
    return (min(float(np.min(np.abs(c - thr) / thr)) for c, _ in read),
            min(float(np.min(np.abs(z))) for _, z in read))


def decisive(r, margin=1e-6):
    """every chi2 decision of both rounds stayed `margin` (relative) from its threshold"""
    return all(m >= margin for tr in r.trace for m in tr.margins)
