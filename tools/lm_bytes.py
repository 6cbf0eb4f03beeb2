"""Every output byte of pose_optimization_batch and optimize_sim3_batch on the
fixtures of tests/test_poseopt.py and tests/test_sim3opt.py, for comparing two
builds of the library: the size sweeps (n = 4100 and CAP + 3 are past what the
kernels keep in LDS), the named cases, and the 64 mixed jobs of the two
test_gpu_batch_invariance_and_determinism (CAP + 40 among them), each group
as one batch.  Writes the result records and flag arrays to one .npz.

Run it once per library, each run a process of its own, and compare:

  ORBGPU_LIBRARY=<a.so> python tools/lm_bytes.py a.npz
  ORBGPU_LIBRARY=<b.so> python tools/lm_bytes.py b.npz
  python tools/lm_bytes.py --compare a.npz b.npz      (no GPU; exit status 1 on any difference)
"""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in ("orb-slam2-annotation_amd", "tests"):
    sys.path.insert(0, str(ROOT / p))


def collect():
    import poseopt
    import sim3opt
    import test_poseopt as tp
    import test_sim3opt as ts

    out = {}
    groups = {"sizes": [tp.scene(**tp.size_scene(n)) for n in tp.SIZE_SEEDS],
              "cases": [tp.scene(**kw) for kw in tp.CASES.values()],
              "mixed": tp._mixed_scenes(64, 700)}
    for name, scenes in groups.items():
        jobs, Xw, obs, w = tp.pack(scenes)
        res, flags = poseopt.pose_optimization_batch(jobs, Xw, obs, w)
        out[f"poseopt_{name}_results"], out[f"poseopt_{name}_flags"] = res.view(np.uint8), flags
    groups = {"sizes": [ts.scene(**ts.size_scene(n)) for n in ts.SIZES],
              "cases": [ts.scene(**kw) for kw in ts.CASES.values()],
              "mixed": ts._mixed_scenes(64, 700)}
    for name, scenes in groups.items():
        jobs, arrays = ts.pack(scenes)
        res, flags = sim3opt.optimize_sim3_batch(jobs, *arrays)
        out[f"sim3opt_{name}_results"], out[f"sim3opt_{name}_flags"] = res.view(np.uint8), flags
    return out


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    same = sorted(a.files) == sorted(b.files)
    for path, z in ((path_a, a), (path_b, b)):  # of the arrays in name order: a .npz also holds time stamps
        h = hashlib.sha256(b"".join(z[k].tobytes() for k in sorted(z.files))).hexdigest()
        print(f"sha256 of the arrays {h}  {path}")
    for k in sorted(a.files):
        eq = k in b.files and a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
        print(f"{k:28s} {a[k].nbytes:8d} bytes  {'equal' if eq else 'DIFFERENT'}")
        same = same and eq
    print("verdict:", "every array equal byte for byte" if same else "the two libraries differ")
    return 0 if same else 1


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    arrays = collect()
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    np.savez(sys.argv[1], **{k: np.ascontiguousarray(v) for k, v in arrays.items()})
    print("wrote", sys.argv[1], {k: v.shape for k, v in arrays.items()})
