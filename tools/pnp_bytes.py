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
The problems are built by tests/pnp_cases.py.  Every byte of a record is written
by the library (a pose the call did not produce is all zeros), so nothing is masked.

Run it once per library, each run a process of its own, and compare:

  ORBGPU_LIBRARY=<a.so> python tools/pnp_bytes.py a.npz
  ORBGPU_LIBRARY=<b.so> python tools/pnp_bytes.py b.npz
  python tools/pnp_bytes.py --compare a.npz b.npz      (no GPU; exit status 1 on any difference)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in ("orb-slam2-annotation_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, str(ROOT / p))


def collect():
    import test_pnp
    from pnp_cases import planar_case, refine_case, repeated_case, six_cases

    out = {}

    def run(name, cases):
        arr, res, bm, rm = test_pnp._run_batch(cases)
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


RECORD = np.dtype([("found", "<i4"), ("consumed", "<i4"), ("best_inliers", "<i4"), ("best_hyp", "<i4"),
                   ("refined_inliers", "<i4"), ("best_Tcw", "<f4", 16), ("refined_Tcw", "<f4", 16)])


def differing_words(path_a, path_b):
    """which fields of which result records differ between two runs, and whether every difference
    lies in a pose the call did not produce (best_Tcw with best_hyp < 0, refined_Tcw without found):
    the words that a library from before the zero-pose convention left unwritten"""
    a, b = np.load(path_a), np.load(path_b)
    only_absent_poses = True
    for k in sorted(f for f in a.files if f.endswith("_results")):
        ra, rb = a[k].view(RECORD), b[k].view(RECORD)
        for i, (x, y) in enumerate(zip(ra, rb)):
            fields = [f for f in RECORD.names if np.asarray(x[f]).tobytes() != np.asarray(y[f]).tobytes()]
            if not fields:
                continue
            absent = all((f == "best_Tcw" and x["best_hyp"] < 0 and y["best_hyp"] < 0) or
                         (f == "refined_Tcw" and not x["found"] and not y["found"]) for f in fields)
            only_absent_poses = only_absent_poses and absent
            print(f"{k}[{i}]: {', '.join(fields)} differ{' (a pose the call did not produce)' if absent else ''}")
    print("result records: " + ("the only differing words are poses the call did not produce" if only_absent_poses
                                else "words that the call produced DIFFER"))


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        from lm_bytes import compare
        differing_words(sys.argv[2], sys.argv[3])
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
