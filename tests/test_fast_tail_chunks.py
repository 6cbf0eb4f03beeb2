"""FAST arc pass with the 64-entry tail chunk (csrc/fast.hip: arc_chunk while
65 or more survivors remain, then arc_chunk_half for 1 .. 64): per-level FAST
candidates and the full extraction, bit for bit against the oracle, on frames
whose per-cell survivor counts sweep from 0 to past the survivor list.

Texture: uniform noise whose amplitude ramps from 0 at the left edge to 127 at
the right one (amplitude ~ (x / (w - 1)) ** gamma), so cell columns go from no
compass survivor to nearly every pixel.  Seeds and gammas were picked on the
CPU so that the oracle's levels alone satisfy the coverage asserts below (the
survivor counts come from the numpy compass formula of
tools/fast_cell_stats.py, before the GPU is touched):

* 640x480 (windows of 48 x 40 bytes; survivor list 496 entries, shorter than
  a level-0 cell's 992 pixels: cells past it take more than one row band), and
* 1241x376 (windows of 48 x 46 bytes, the same pitch template; the list holds
  a whole cell, 1280 entries, so every cell is one band and the arc pass runs
  up to 7 chunks in a row).
"""
import functools

import numpy as np
import pytest

import orbref
from tools.fast_cell_stats import cell_survivors, list_len

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

#         w,    h,   nfeatures, seed, gamma, a level-0 cell overflows the list
FRAMES = {"640x480": (640, 480, 1000, 18, 1.0, True),
          "1241x376": (1241, 376, 2000, 23, 1.5, False)}
TAILS = {0, 1, 63, 64, 65, 127}             # s % 128 (s >= 1): chunk-boundary tails
COUNTS = {1, 64, 65, 128, 129, 192, 193}    # s itself: 0 / 1 / 2 full chunks with and without a tail


def ramp_noise(w, h, seed, gamma):
    rng = np.random.default_rng(seed)
    ramp = (np.arange(w) / (w - 1.0)) ** gamma
    n = rng.uniform(-1.0, 1.0, (h, w))
    return np.clip(np.rint(128.0 + 127.0 * ramp[None, :] * n), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(image, oracle keypoints, descriptors, per-level candidates), computed
    once per frame, with the coverage of the chunk-boundary cases asserted on
    the oracle's levels"""
    w, h, nf, seed, gamma, overflows = FRAMES[name]
    img = ramp_noise(w, h, seed, gamma)
    ref = orbref.Extractor(nfeatures=nf)
    kr, dr = ref.extract(img)
    levels = [ref.level(l) for l in range(8)]
    s = [cell_survivors(im, 20) for im in levels]  # compass survivors per cell at iniThFAST
    alls = np.concatenate(s)
    assert alls.min() == 0 and alls.max() > 256
    missing = TAILS - set((alls[alls >= 1] % 128).tolist())
    assert not missing, f"no cell with s % 128 in {sorted(missing)}"
    missing = COUNTS - set(alls.tolist())
    assert not missing, f"no cell with s in {sorted(missing)}"
    dump = list_len([(im.shape[1], im.shape[0]) for im in levels])
    assert bool((s[0] > dump).any()) == overflows, (dump, int(s[0].max()))
    return img, kr, dr, [ref.candidates(l) for l in range(8)]


def _gpu():
    import orbgpu
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return orbgpu


def test_frames_cover_the_boundary_cases():
    """every frame reaches every chunk-boundary case (asserted in _oracle), and
    in at least one a level-0 cell overflows the list: more than one row band"""
    assert any(f[5] for f in FRAMES.values())
    for name in FRAMES:
        _oracle(name)


@pytest.mark.parametrize("name", list(FRAMES))
def test_candidates_per_level(name):
    img, _, _, cands = _oracle(name)
    og = _gpu()
    w, h, nf = FRAMES[name][:3]
    ex = og.Extractor(nfeatures=nf, width=w, height=h)
    ex.extract(img)
    for l in range(8):
        cg, cr = ex.candidates(l), cands[l]
        assert cg.shape == cr.shape, f"level {l}: {len(cg)} vs {len(cr)} candidates"
        np.testing.assert_array_equal(cg, cr, err_msg=f"candidates level {l}")


@pytest.mark.parametrize("name", list(FRAMES))
def test_full_extraction(name):
    img, kr, dr, _ = _oracle(name)
    og = _gpu()
    w, h, nf = FRAMES[name][:3]
    ex = og.Extractor(nfeatures=nf, width=w, height=h)
    kg, dg = ex.extract(img)
    assert len(kg) == len(kr) > 0, (len(kg), len(kr))
    assert kg.tobytes() == kr.tobytes(), "keypoints differ from the oracle"
    assert np.array_equal(dg, dr), "descriptors differ from the oracle"
