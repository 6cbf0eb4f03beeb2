"""Every byte of orbgpu_pnp_ransac_batch's result records and of both masks, for
comparing two builds of the library, over
  * the 16 cases of tests/test_pnp.py::test_pnp_gpu_batch_vs_oracle, one batch;
  * six problems with n = 12 .. 300 and n_hyp = 1, 2, 3, 5, 64, 130 (a lone group, partial
    waves, more than one block), as one batch and each alone (--compare also says whether a
    problem computed the same alone as in the batch);
  * the paths the suite does not reach (here the oracle keeps rounding-defined
    eigenvectors and is no judge; only two builds can be compared):
      repeated  3D points given twice, with samples that pick both copies: the
                minimal set's 12 x 12 system is singular and the wave takes the
                eigen path with k = 4 null vectors to canonicalise;
      planar    all points on one plane;
      refine4/5/6  min_inliers = 4 and exactly 4, 5, 6 inliers: Refine runs EPnP
                on them (k = 4, 2, 0 null vectors to canonicalise).
The unwritten words of a record (the refined pose of a problem that found none,
the best pose of one with no best) are zeroed: they hold whatever the arena held.

Run it once per library, each run a process of its own, and compare:

  ORBGPU_LIBRARY=<a.so> python tools/pnp_bytes.py a.npz
  ORBGPU_LIBRARY=<b.so> python tools/pnp_bytes.py b.npz
  python tools/pnp_bytes.py --compare a.npz b.npz      (no GPU; exit status 1 on any difference)
"""
import ctypes
import sys
from itertools import combinations
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in ("orb-slam2-annotation_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, str(ROOT / p))


def _project(P, X):
    fu, fv, uc, vc = P["cam"]
    Xc = X.astype(np.float64) @ P["R"].T + P["t"]
    return np.stack([uc + fu * Xc[:, 0] / Xc[:, 2], vc + fv * Xc[:, 1] / Xc[:, 2]], 1)


def _samples(rng, n, count):
    return np.stack([rng.choice(n, 4, replace=False) for _ in range(count)]).astype(np.int32)


def six_cases():
    import synth
    rng = np.random.default_rng(31)
    out = []
    for b, (n, n_hyp) in enumerate(zip([12, 40, 80, 120, 200, 300], [1, 2, 3, 5, 64, 130])):
        P = synth.pnp_problem(n, [0.0, 0.3, 0.5, 0.8, 1.0][b % 5], seed=400 + b)
        out.append((P, _samples(rng, n, n_hyp), max(int(np.float32(n) * np.float32(0.5)), 10)))
    return out


def repeated_case():
    import synth
    P = synth.pnp_problem(60, 0.8, seed=611)
    for d, s in ((1, 0), (3, 2), (5, 4)):
        P["P3w"][d], P["P2"][d], P["sigma2"][d] = P["P3w"][s], P["P2"][s], P["sigma2"][s]
    rng = np.random.default_rng(612)
    twice = np.array([[0, 1, 7, 9], [2, 3, 0, 1], [4, 5, 2, 3], [10, 0, 11, 1]], np.int32)
    return P, np.concatenate([twice, _samples(rng, 60, 40), twice[::-1]]), 30


def planar_case():
    import synth
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


def refine_case(k):
    """exactly k inliers (noise-free, the first k points) among 30, min_inliers = 4, every 4-subset
    of the inliers sampled first: the first seed at which the oracle's first hypothesis has exactly
    k inliers, so Refine's EPnP runs on k correspondences"""
    import pnp_ref
    import synth
    for seed in range(700, 760):
        P = synth.pnp_problem(30, 0.0, seed=seed)
        P["P2"][:k] = _project(P, P["P3w"][:k]).astype(np.float32)
        P["sigma2"][:] = np.float32(1.2) ** 6
        samples = np.concatenate([np.array(list(combinations(range(k), 4)), np.int32),
                                  _samples(np.random.default_rng(seed), 30, 8)])
        o = pnp_ref.ransac_call(P["P3w"], P["P2"], P["sigma2"] * np.float32(5.991), P["cam"], 4, 0,
                                np.zeros(30, bool), samples[:1])
        if o["best_inliers"] == k:
            return P, samples, 4
    raise AssertionError(f"no seed with exactly {k} inliers")


def collect():
    import ransac
    import test_pnp

    out = {}

    def run(name, cases):
        arr, res, bm, rm = test_pnp._run_batch(cases)
        for r in res:
            if not r.found:
                ctypes.memset(ctypes.addressof(r) + ransac.PnPResult.refined_Tcw.offset, 0, 64)
            if r.best_hyp < 0:
                ctypes.memset(ctypes.addressof(r) + ransac.PnPResult.best_Tcw.offset, 0, 64)
        out[f"{name}_results"] = np.frombuffer(bytes(res), np.uint8).copy()
        out[f"{name}_best_mask"], out[f"{name}_refined_mask"] = bm, rm
        print(name, [(r.found, r.consumed, r.best_inliers, r.refined_inliers) for r in res])

    run("oracle16", test_pnp._oracle_cases())
    six = six_cases()
    run("six", six)
    for b, case in enumerate(six):
        run(f"six_alone{b}", [case])
    run("repeated", [repeated_case()])
    run("planar", [planar_case()])
    for k in (4, 5, 6):
        run(f"refine{k}", [refine_case(k)])
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        from lm_bytes import compare
        for path in sys.argv[2:4]:
            z, n_off = np.load(path), 0
            for b, n in enumerate([12, 40, 80, 120, 200, 300]):
                same = (z["six_results"][148 * b:148 * (b + 1)].tobytes() == z[f"six_alone{b}_results"].tobytes() and
                        all(z[f"six_{m}_mask"][n_off:n_off + n].tobytes() == z[f"six_alone{b}_{m}_mask"].tobytes()
                            for m in ("best", "refined")))
                print(f"{path}: problem {b} of the six alone {'equals' if same else 'DIFFERS from'} its batch run")
                n_off += n
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    arrays = collect()
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    np.savez(sys.argv[1], **{k: np.ascontiguousarray(v) for k, v in arrays.items()})
    print("wrote", sys.argv[1], {k: v.shape for k, v in arrays.items()})
