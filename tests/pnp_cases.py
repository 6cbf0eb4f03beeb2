"""Problems for orbgpu_pnp_ransac_batch: the builders of tests/test_pnp.py and tools/pnp_bytes.py.

A case is (P, samples, min_inliers) or (P, samples, min_inliers, best_inliers, best_mask): P is a
synth.pnp_problem dict, samples the (n_hyp, 4) minimal sets, best_inliers and best_mask the state
carried into the call (mnBestInliers and mvbBestInliers; 0 and all-zero when left out).
`oracle(case)` is pnp_ref.ransac_call on it.  Builders and their oracle results are computed once
per process (functools.lru_cache): treat what they return as read-only."""
from functools import lru_cache
from itertools import combinations

import numpy as np

import pnp_ref
import synth


def _project(P, X):
    fu, fv, uc, vc = P["cam"]
    Xc = X.astype(np.float64) @ P["R"].T + P["t"]
    return np.stack([uc + fu * Xc[:, 0] / Xc[:, 2], vc + fv * Xc[:, 1] / Xc[:, 2]], 1)


def _samples(rng, n, count):
    return np.stack([rng.choice(n, 4, replace=False) for _ in range(count)]).astype(np.int32)


def maxerr(P):
    return P["sigma2"] * np.float32(5.991)


def oracle(case):
    """pnp_ref.ransac_call on a case"""
    P, samples, min_inl = case[:3]
    n = len(P["P3w"])
    best, mask = (case[3], case[4]) if len(case) > 3 else (0, np.zeros(n, bool))
    return pnp_ref.ransac_call(P["P3w"], P["P2"], maxerr(P), P["cam"], min_inl, best, np.asarray(mask, bool),
                               samples)


def outcome(o):
    return o["found"], o["consumed"], o["best_hyp"], o["best_inliers"]


def six_cases():
    rng = np.random.default_rng(31)
    out = []
    for b, (n, n_hyp) in enumerate(zip([12, 40, 80, 120, 200, 300], [1, 2, 3, 5, 64, 130])):
        P = synth.pnp_problem(n, [0.0, 0.3, 0.5, 0.8, 1.0][b % 5], seed=400 + b)
        out.append((P, _samples(rng, n, n_hyp), max(int(np.float32(n) * np.float32(0.5)), 10)))
    return out


def repeated_case():
    P = synth.pnp_problem(60, 0.8, seed=611)
    for d, s in ((1, 0), (3, 2), (5, 4)):
        P["P3w"][d], P["P2"][d], P["sigma2"][d] = P["P3w"][s], P["P2"][s], P["sigma2"][s]
    rng = np.random.default_rng(612)
    twice = np.array([[0, 1, 7, 9], [2, 3, 0, 1], [4, 5, 2, 3], [10, 0, 11, 1]], np.int32)
    return P, np.concatenate([twice, _samples(rng, 60, 40), twice[::-1]]), 30


def planar_case():
    P = synth.pnp_problem(80, 0.8, seed=621)
    X = P["P3w"].astype(np.float64)
    before = _project(P, X)
    nrm = P["R"].T @ np.array([0.3, -0.2, 1.0])  # a plane tilted against the image plane
    nrm /= np.linalg.norm(nrm)
    c = X.mean(0)
    X = X - np.outer((X - c) @ nrm, nrm)
    P["P3w"] = X.astype(np.float32)
    inl = P["inlier"]
    P["P2"][inl] = (_project(P, P["P3w"]) + (P["P2"].astype(np.float64) - before))[inl].astype(np.float32)
    return P, _samples(np.random.default_rng(622), 80, 60), 40


@lru_cache(maxsize=None)
def refine_case(k):
    """exactly k inliers (noise-free, the first k points) among 30, min_inliers = 4, every 4-subset
    of the inliers sampled first: the first seed at which the oracle's first hypothesis has exactly
    k inliers, so Refine's EPnP runs on k correspondences"""
    for seed in range(700, 760):
        P = synth.pnp_problem(30, 0.0, seed=seed)
        P["P2"][:k] = _project(P, P["P3w"][:k]).astype(np.float32)
        P["sigma2"][:] = np.float32(1.2) ** 6
        samples = np.concatenate([np.array(list(combinations(range(k), 4)), np.int32),
                                  _samples(np.random.default_rng(seed), 30, 8)])
        o = pnp_ref.ransac_call(P["P3w"], P["P2"], maxerr(P), P["cam"], 4, 0, np.zeros(30, bool), samples[:1])
        if o["best_inliers"] == k:
            return P, samples, 4
    raise AssertionError(f"no seed with exactly {k} inliers")


# ---- the best returned without a refined pose ----------------------------------------------
HELD_K = (4, 5, 6, 10)
HELD_OUTCOME = {4: (0, 9, 0, 4), 5: (0, 13, 0, 5), 6: (0, 23, 0, 6), 10: (0, 218, 0, 10)}


def held_best_case(k):
    """refine_case(k) with min_inliers = k: Refine never has MORE than k inliers, so the call runs
    out of hypotheses holding hypothesis 0 as its best, and iterate() returns mBestTcw"""
    P, samples, _ = refine_case(k)
    return P, samples, k


def padded_case():
    """held_best_case(6) with its samples padded to 300: the replay crosses the LDS chunk of 256
    hypothesis counts holding its best"""
    P, samples, _ = refine_case(6)
    return P, np.concatenate([samples, _samples(np.random.default_rng(1), 30, 300 - len(samples))]), 6


PADDED_OUTCOME = (0, 300, 0, 6)


@lru_cache(maxsize=None)
def padded_oracle():
    return oracle(padded_case())


# ---- state carried from one call into the next ----------------------------------------------
CARRIED_OUTCOME = ((0, 7, 0, 6), (0, 293, -1, 6), (1, 1, -1, 6))


def carried_cases(best_inliers, best_mask):
    """padded_case() as two calls: its first 7 hypotheses, then (given what the first call left) the
    other 293 with the state carried in, and those again with min_inliers = 5: the first of them
    qualifies without beating the best, so Refine runs on the carried mask and succeeds"""
    P, samples, min_inl = padded_case()
    return ((P, samples[:7], min_inl), (P, samples[7:], min_inl, best_inliers, best_mask),
            (P, samples[7:], 5, best_inliers, best_mask))


@lru_cache(maxsize=None)
def carried_oracles():
    o1 = oracle(carried_cases(0, None)[0])
    _, c2, c3 = carried_cases(o1["best_inliers"], o1["best_mask"].astype(np.uint8))
    return o1, oracle(c2), oracle(c3)


# ---- the first qualifying hypothesis on either side of the chunk boundary ------------------
CHUNK = ((41, 255), (42, 256), (45, 255), (48, 299), (44, 299))
CHUNK_OUTCOME = {(41, 255): (1, 257, 256), (42, 256): (1, 258, 257), (45, 255): (1, 256, 255),
                 (48, 299): (1, 300, 299), (44, 299): (0, 300, -1)}  # found, consumed, best_hyp


@lru_cache(maxsize=None)
def chunk_case(seed, K):
    """K minimal sets of outliers (each scores <= 1 in the oracle), then 300 - K of inliers"""
    P = synth.pnp_problem(120, 0.7, seed)
    rng = np.random.default_rng(seed)
    out_idx, in_idx = np.nonzero(~P["inlier"])[0], np.nonzero(P["inlier"])[0]
    samples = [rng.choice(out_idx, 4, replace=False) for _ in range(K)]
    samples += [rng.choice(in_idx, 4, replace=False) for _ in range(300 - K)]
    return P, np.stack(samples).astype(np.int32), 60


@lru_cache(maxsize=None)
def chunk_oracle(seed, K):
    return oracle(chunk_case(seed, K))


# ---- Refine on a chosen set -----------------------------------------------------------------
REFINE_M = (4, 5, 6, 7, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 256, 257, 320)


@lru_cache(maxsize=None)
def refine_set_case(m):
    """320 noise-free points, an incoming best of "320" whose mask is m chosen points, min_inliers 0
    and one hypothesis: it qualifies, does not beat the best, and the loop body runs Refine on
    exactly the chosen m"""
    P = synth.pnp_problem(320, 1.0, seed=900 + m, noise_px=0.0)
    mask = np.zeros(320, np.uint8)
    mask[np.sort(np.random.default_rng(m).choice(320, m, replace=False))] = 1
    return P, np.array([[0, 1, 2, 3]], np.int32), 0, 320, mask


# ---- every hypothesis, one per problem ------------------------------------------------------
@lru_cache(maxsize=None)
def single_hyp_sets():
    """(P, sets, counts): 64 minimal sets on 60 points, and the oracle's CheckInliers count of each"""
    P = synth.pnp_problem(60, 1.0, seed=77)
    sets = _samples(np.random.default_rng(5), 60, 64)
    pw, us = P["P3w"].astype(np.float64), P["P2"].astype(np.float64)
    cam = tuple(float(c) for c in P["cam"])
    counts = []
    for idx in sets:
        R, t, _ = pnp_ref.compute_pose(pw[idx], us[idx], cam)
        counts.append(int(pnp_ref.check_inliers(R, t, P["P3w"], P["P2"], maxerr(P), cam).sum()))
    return P, sets, np.array(counts)


# ---- a regular set beside degenerate ones ---------------------------------------------------
@lru_cache(maxsize=None)
def eigen_path_cases():
    """([X, D, D', D''], [X, r, r', r'']) on repeated_case's points.  X: four distinct points, the
    first draw that the oracle accepts and refines at once.  D: sets holding both copies of a
    repeated 3D point, whose 12 x 12 system is singular, so the wave they share with X takes the
    eigen path.  r: regular sets."""
    P = repeated_case()[0]
    rng = np.random.default_rng(613)
    single = np.arange(6, 60)  # points 0 .. 5 are the three repeated pairs
    X = None
    for _ in range(20):
        cand = rng.choice(single, 4, replace=False).astype(np.int32)
        if outcome(oracle((P, cand[None], 30)))[:3] == (1, 1, 0):
            X = cand
            break
    assert X is not None
    D = np.array([[0, 1, 7, 9], [2, 3, 0, 1], [4, 5, 2, 3]], np.int32)
    r = np.stack([rng.choice(single, 4, replace=False) for _ in range(3)]).astype(np.int32)
    return (P, np.concatenate([X[None], D]), 30), (P, np.concatenate([X[None], r]), 30)
