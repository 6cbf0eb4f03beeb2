"""The octree's fused first passes (csrc/octree.hip: one key sweep, the main
passes 1-3 replayed on per-(root, path) counts) against the CPU oracle, per
level and per frame, exact: the outputs are integers.

Each case is named for the branch it takes.  Which branch a level takes is
read from the oracle's candidates with tests/octree_passes_ref.py -- a plain
restatement of the fused passes, itself checked against the oracle here on
the CPU -- and, on the GPU, from the kernel's trace word for frame 0.

Batch sizes: 1 and 3 run the 1024-thread kernel (batches up to 8 do), 9 the
256-thread kernel; the frames of a batch are distinct.
"""
import functools

import numpy as np
import pytest

import octree_passes_ref as passes
import orbref
import synth

LEVELS = 8


def _textured(w=640, h=480, seed=5):
    return synth.mono_stream(1, w, h, seed=seed)[0]


def _quadrant():
    img = synth.flat_image().copy()
    img[:240, :320] = _textured()[:240, :320]
    return img


def _quadrant_and_patch():
    # the top-left quadrant and a patch inside the top-right one: the root keeps two of its
    # four children, and the patch's quadrant in turn only some of its own
    img = _quadrant()
    img[40:150, 500:600] = _textured()[40:150, 500:600]
    return img


def _blobs():
    img = synth.flat_image().copy()
    img[200:204, 300:304] = 255
    img[90:93, 520:523] = 0
    return img


# name -> (image, nfeatures, what frame 0's levels must show: a predicate over the per-level branch records)
CASES = {
    "three_passes": (_textured, 1000, lambda r: all(i["replayed"] == 3 and i["inner"] for i in r[:7])),
    "finish_at_pass_2": (_textured, 40, lambda r: all(i["replayed"] == 1 and i["inner"] for i in r[:4])),
    "finish_at_pass_3": (_textured, 150, lambda r: all(i["replayed"] == 2 and i["inner"] for i in r[:4])),
    # every key in one quadrant: pass 1 leaves the list at one node, which ends the distribution
    "one_quadrant": (_quadrant, 1000, lambda r: all(i["replayed"] == 0 and i["sizes"] == [1] for i in r)),
    "children_dropped": (_quadrant_and_patch, 1000,
                         lambda r: any(i["replayed"] == 3 and i["dropped"][0] and i["dropped"][1] for i in r)),
    "hbm_key_store": (synth.noise_image, 1000, lambda r: r[0]["nk"] > 4096 and r[0]["replayed"] == 3),
    "no_keys": (synth.flat_image, 1000, lambda r: all(i["nk"] == 0 for i in r)),
    "one_to_three_keys": (_blobs, 1000, lambda r: {i["nk"] for i in r} >= {1, 2} and max(i["nk"] for i in r) <= 3),
    "several_roots": (lambda: _textured(1241, 376, 21), 2000,
                      lambda r: all(i["roots"] == 4 for i in r) and r[0]["replayed"] == 3 and r[0]["sizes"][2] > 64),
    # more roots than the fused scratch holds: the level goes pass by pass
    "many_roots": (lambda: _textured(2000, 300, 33), 1000, lambda r: all(i["roots"] >= 7 and not i["fused"] for i in r)),
}


def _variant(img, b):
    """Frame b of a case's batch: flips and the negative, all of the same structure."""
    v = [img, img[:, ::-1], img[::-1, :], img[::-1, ::-1]][b % 4]
    return np.ascontiguousarray(255 - v if (b // 4) % 2 else v)


@functools.lru_cache(maxsize=None)
def _oracle(name, b):
    """(candidates, octree output) per level, features per level, of frame b of a case (computed once)."""
    make, nf, _ = CASES[name]
    ref = orbref.Extractor(nfeatures=nf)
    ref.extract(_variant(make(), b))
    return ([ref.candidates(l) for l in range(LEVELS)], [ref.octree(l) for l in range(LEVELS)],
            [int(n) for n in ref.features_per_level()])


@functools.lru_cache(maxsize=None)
def _branches(name):
    """Per level of frame 0: the fused passes' record, from the oracle's candidates."""
    make, _, _ = CASES[name]
    h, w = make().shape
    cands, octs, N = _oracle(name, 0)
    geo = passes.level_geometry(w, h)
    out = []
    for l in range(LEVELS):
        for fused in (False, True):  # (the record kept is the fused form's)
            keys, info = passes.distribute(cands[l], geo[l][0], geo[l][1], N[l], fused=fused)
            np.testing.assert_array_equal(keys, octs[l], err_msg=f"{name} level {l} fused={fused}: restatement")
        out.append(dict(info, nk=len(cands[l])))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_case_takes_its_branch(name):
    """CPU: the restated passes (fused and pass by pass) equal the oracle on every
    level, and the case's frame 0 takes the branch the case is named for."""
    rec = _branches(name)
    assert CASES[name][2](rec), [{k: i[k] for k in ("nk", "replayed", "inner", "sizes", "dropped", "roots")} for i in rec]


def test_fused_scratch_fits_a_pass_of_64_nodes():
    """The restatement's bounds, as the kernel's scratch assumes them: up to four
    roots, so at most 64 nodes before pass 3 and at most 256 after it."""
    for name in CASES:
        for i in _branches(name):
            assert i["roots"] <= 4 or not i["fused"]
            before = [i["roots"]] + i["sizes"]
            assert all(before[p] <= 64 and before[p + 1] <= 256 for p in range(i["replayed"]))


def test_octree_plan_keeps_six_workgroups_and_fits_the_fused_scratch():
    """Host side (no GPU): the fused sweep's scratch (2880 B: counts of 4 roots x
    84 bins, the bin table, two tag lists) lies over the quadrant counters, aux
    words and flags (17 B per node).  At 640x480 / 1000 features those are larger,
    so the launch keeps its LDS, key capacity and six workgroups per 160 KiB CU;
    with few nodes the scratch sets the floor, and the keys still follow it."""
    import orbgpu
    a, b = orbgpu.octree_plan(1000, 1.2, 8, 640, 480)
    assert (a["level0"], a["levels"], b["level0"], b["levels"]) == (0, 2, 2, 6)
    assert a["ncap"] == 224 and a["kcap"] == 2560 and 17 * a["ncap"] >= 2880
    fixed = 128 + 2 * 16 * a["ncap"]  # misc, the two node lists (the cell offsets fit in the second)
    assert a["lds_bytes"] == fixed + 17 * a["ncap"] + 6 * a["kcap"] == 26464
    assert 6 * max(a["lds_bytes"], b["lds_bytes"]) <= 160 * 1024
    for nf in (40, 150):
        for g in orbgpu.octree_plan(nf, 1.2, 8, 640, 480):
            assert 17 * g["ncap"] < 2880
            cells = g["lds_bytes"] - 128 - 16 * g["ncap"] - 2880 - 6 * g["kcap"]  # node list 1 | cell offsets
            assert cells >= 16 * g["ncap"] and g["lds_bytes"] <= 65536


def _run_gpu(name, B, trace=False):
    torch = pytest.importorskip("torch")
    import orbgpu
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    make, nf, _ = CASES[name]
    img = make()
    h, w = img.shape
    frames = np.stack([_variant(img, b) for b in range(B)])
    ex = orbgpu.Extractor(nfeatures=nf, width=w, height=h, max_batch=B)
    if trace:
        ex.enable_octree_trace()
    pitch = (w + 15) // 16 * 16  # (rows 16-byte aligned, as the device path asks)
    padded = np.zeros((B, h, pitch), np.uint8)
    padded[:, :, :w] = frames
    imgs = torch.from_numpy(padded).cuda()[:, :, :w]
    cap = ex.max_keypoints
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch(imgs, kps, desc, counts)
    ex.sync()
    for b in range(B):
        cands, octs, _ = _oracle(name, b)
        for l in range(LEVELS):
            cg = ex.candidates(l, b)
            assert cg.shape == cands[l].shape and np.array_equal(cg, cands[l]), f"frame {b} level {l}: candidates"
            og = ex.octree(l, b)
            assert og.shape == octs[l].shape, f"frame {b} level {l}: octree {len(og)} vs {len(octs[l])} keys"
            np.testing.assert_array_equal(og, octs[l], err_msg=f"frame {b} level {l}: octree")
    return ex


def _trace_word(ex):
    raw = np.zeros(16 * 512, np.int32)
    import orbgpu
    orbgpu._check(orbgpu.lib().orbgpu_debug_octree_trace(ex.h, 0, raw.ctypes.data, raw.size), "octree_trace")
    return [int(raw[l * 512 + 1]) for l in range(LEVELS)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_octree_matches_oracle(name, B):
    """Keys and count of every level of every frame equal the oracle's; frame 0's
    levels took the fused passes the restatement predicts (trace word: 1 + passes
    replayed, 0 for a level on the pass-by-pass path: one without keys or with more
    than four roots)."""
    ex = _run_gpu(name, B, trace=True)
    want = [1 + i["replayed"] if i["fused"] else 0 for i in _branches(name)]
    assert _trace_word(ex) == want


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("name", ["three_passes", "children_dropped", "several_roots"])
def test_pass_by_pass_knob_matches_oracle(monkeypatch, name, B):
    """ORBGPU_OCT_FUSED=0: the same results from the pass-by-pass main loop."""
    monkeypatch.setenv("ORBGPU_OCT_FUSED", "0")
    ex = _run_gpu(name, B, trace=True)
    assert _trace_word(ex) == [0] * LEVELS
