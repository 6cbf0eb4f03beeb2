"""RGB-D input (include/orbgpu_rgbd.h): colour-to-grey of a batch of frames,
and depth lookup / mvuRight / mvDepth / x3Dc at the keypoints, against the
numpy restatement (tests/rgbd_ref.py).  Every comparison is byte-for-byte:
no tolerance, no element left out."""
import ctypes

import numpy as np
import pytest

import orbgpu
import rgbd_ref

# Examples/RGB-D/TUM1.yaml
TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989,
            dist=[0.262383, -0.953104, -0.005358, 0.002628, 1.163314])
K = (TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"])
BF = 40.0
CODES = [orbgpu.COLOR_RGB, orbgpu.COLOR_BGR, orbgpu.COLOR_RGBA, orbgpu.COLOR_BGRA]
F32 = np.float32


# ---------------------------------------------------------------- CPU: restatement pins

def _gray1(px, code=rgbd_ref.COLOR_RGB):
    return int(rgbd_ref.gray_from_color(np.array([px], np.uint8), code)[0])


def test_ref_gray_pins():
    assert _gray1((255, 255, 255)) == 255 and _gray1((0, 0, 0)) == 0
    assert _gray1((1, 0, 0)) == 0 and _gray1((2, 0, 0)) == 1  # (R*4899 + 8192) >> 14: the rounding term
    assert (_gray1((255, 0, 0)), _gray1((0, 255, 0)), _gray1((0, 0, 255))) == (76, 150, 29)
    assert rgbd_ref.gray_from_color(np.zeros((2, 3, 5, 3), np.uint8), rgbd_ref.COLOR_RGB).shape == (2, 3, 5)


def test_ref_gray_codes_agree_after_permutation_and_alpha_is_ignored():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (7, 11, 3), dtype=np.uint8)
    want = rgbd_ref.gray_from_color(rgb, rgbd_ref.COLOR_RGB)
    bgr = rgb[..., ::-1]
    assert np.array_equal(rgbd_ref.gray_from_color(bgr, rgbd_ref.COLOR_BGR), want)
    for alpha in (0, 255, None):
        a = rng.integers(0, 256, (7, 11, 1), dtype=np.uint8) if alpha is None else np.full((7, 11, 1), alpha, np.uint8)
        assert np.array_equal(rgbd_ref.gray_from_color(np.concatenate([rgb, a], 2), rgbd_ref.COLOR_RGBA), want)
        assert np.array_equal(rgbd_ref.gray_from_color(np.concatenate([bgr, a], 2), rgbd_ref.COLOR_BGRA), want)
    assert not np.array_equal(rgbd_ref.gray_from_color(rgb, rgbd_ref.COLOR_BGR), want)


def _one(depth_map, factor, x, y, ux=None, uy=None, bf=BF):
    ux = x if ux is None else ux
    uy = y if uy is None else uy
    u, d, p = rgbd_ref.stereo_from_rgbd(depth_map, factor, [x], [y], [ux], [uy], K, bf)
    return u[0], d[0], p[0]


def test_ref_depth_pins():
    m = np.zeros((4, 16), np.uint16)
    m[2, 10], m[2, 11] = 5000, 7
    f = F32(1.0) / F32(5000.0)
    u, d, p = _one(m, f, 10.999, 2.999, ux=12.5, uy=3.25)  # truncation, not rounding: column 10, row 2
    want = F32(5000) * f
    assert d.tobytes() == want.tobytes()
    assert u.tobytes() == (F32(12.5) - F32(BF) / want).tobytes()
    fx, fy, cx, cy = (F32(v) for v in K)
    assert p.tobytes() == np.array([(F32(12.5) - cx) * want * (F32(1) / fx), (F32(3.25) - cy) * want * (F32(1) / fy),
                                    want], F32).tobytes()
    assert _one(m, f, 11.0, 2.0)[1] == F32(7) * f
    assert _one(m, 1.0, 10.0, 2.0)[1] == F32(5000)  # u16 is always converted
    g = np.zeros((4, 16), F32)
    g[1, 3], g[1, 4], g[1, 5], g[1, 6], g[1, 7] = 2.5, 0.0, -1.0, np.nan, 1e-30
    assert _one(g, 1.0, 3.5, 1.5)[1].tobytes() == F32(2.5).tobytes()
    # |factor - 1| <= 1e-5: Tracking.cpp:264 skips convertTo, the sample is passed through unscaled
    assert _one(g, 1.000005, 3.5, 1.5)[1].tobytes() == F32(2.5).tobytes()
    assert _one(g, 1.0, 7.0, 1.0)[1].tobytes() == F32(1e-30).tobytes()
    assert _one(g, 0.5, 3.5, 1.5)[1].tobytes() == F32(1.25).tobytes()
    assert _one(g, 1.00002, 3.5, 1.5)[1].tobytes() == (F32(2.5) * F32(1.00002)).tobytes()
    for col in (4, 5, 6):  # 0, -1 and NaN
        for factor in (1.0, 0.5):
            u, d, p = _one(g, factor, float(col), 1.0)
            assert (u, d) == (-1.0, -1.0) and not p.any()
    for x, y in ((16.0, 1.0), (19.0, 1.0), (3.0, 4.0), (3.0, -2.0), (-1.5, 1.0), (np.nan, 1.0)):  # outside the map
        u, d, p = _one(g, 1.0, x, y)
        assert (u, d) == (-1.0, -1.0) and not p.any()
    assert _one(g, 1.0, -0.5, 1.0)[1] == -1.0 and _one(g, 1.0, 3.0, 1.0)[1] == F32(2.5)  # (int)-0.5 == 0: inside


# ---------------------------------------------------------------- CPU: argument checks of the library

def _gray_call(color=1 << 12, code=0, width=16, height=2, batch=1, srs=48, sfs=96, gray=1 << 13, drs=16, dfs=32):
    return orbgpu.lib().orbgpu_gray_from_color_batch_device(color, code, width, height, batch, srs, sfs, gray, drs,
                                                            dfs, None)


def test_gray_argument_checks_need_no_device():
    """rejected before the device is looked at; the pointers are never dereferenced"""
    E = orbgpu.ERR_ARG
    assert _gray_call(color=None) == E and _gray_call(gray=None) == E
    assert _gray_call(code=4) == E and _gray_call(code=-1) == E
    assert _gray_call(width=0) == E and _gray_call(height=0) == E and _gray_call(batch=-1) == E
    assert _gray_call(srs=47) == E  # src_row_step < width * channels
    assert _gray_call(code=orbgpu.COLOR_BGRA, srs=63) == E
    assert _gray_call(drs=15) == E
    assert _gray_call(batch=2, sfs=95) == E and _gray_call(batch=2, dfs=31) == E
    assert "row" in orbgpu.last_error() or "frame" in orbgpu.last_error()
    assert _gray_call(batch=0) == orbgpu.OK
    assert _gray_call(batch=0, code=orbgpu.COLOR_RGBA, srs=64) == orbgpu.OK


def _depth_call(**kw):
    cam = orbgpu.Camera.make(*K, TUM1["dist"])
    a = dict(maps=1 << 12, dtype=0, factor=1.0, width=16, height=2, rs=32, fs=64, batch=1, kps=1 << 13,
             kps_un=1 << 14, counts=1 << 15, cap=8, cam=ctypes.byref(cam), bf=BF, uright=1 << 16, depth=1 << 17,
             x3dc=None)
    a.update(kw)
    return orbgpu.lib().orbgpu_stereo_from_rgbd_batch_device(
        a["maps"], a["dtype"], a["factor"], a["width"], a["height"], a["rs"], a["fs"], a["batch"], a["kps"],
        a["kps_un"], a["counts"], a["cap"], a["cam"], a["bf"], a["uright"], a["depth"], a["x3dc"], None)


def test_depth_argument_checks_need_no_device():
    E = orbgpu.ERR_ARG
    for name in ("maps", "kps", "kps_un", "counts", "cam", "uright", "depth"):
        assert _depth_call(**{name: None}) == E, name
    assert _depth_call(dtype=2) == E and _depth_call(dtype=-1) == E
    assert _depth_call(width=0) == E and _depth_call(height=0) == E and _depth_call(cap=0) == E
    assert _depth_call(batch=-1) == E
    assert _depth_call(rs=31) == E  # 16 uint16 need 32 bytes
    assert _depth_call(dtype=orbgpu.DEPTH_F32, rs=63, fs=128) == E
    assert _depth_call(batch=2, fs=63) == E
    assert _depth_call(batch=0) == orbgpu.OK
    assert _depth_call(batch=0, dtype=orbgpu.DEPTH_F32, rs=64, fs=128, x3dc=1 << 18) == orbgpu.OK


def test_python_wrappers_reject_wrong_shapes():
    torch = pytest.importorskip("torch")
    gray = torch.zeros((1, 2, 16), dtype=torch.uint8)
    with pytest.raises(ValueError):
        orbgpu.gray_from_color_batch(torch.zeros((1, 2, 16, 4), dtype=torch.uint8), orbgpu.COLOR_RGB, gray)
    with pytest.raises(ValueError):
        orbgpu.gray_from_color_batch(torch.zeros((1, 3, 16, 3), dtype=torch.uint8), orbgpu.COLOR_RGB, gray)
    with pytest.raises(ValueError):
        orbgpu.stereo_from_rgbd_batch(torch.zeros((1, 2, 16), dtype=torch.float64), 1.0, None, None, None, None, BF,
                                      None, None)
    assert (orbgpu.COLOR_RGB, orbgpu.COLOR_BGR, orbgpu.COLOR_RGBA, orbgpu.COLOR_BGRA) == (0, 1, 2, 3)
    assert (orbgpu.DEPTH_U16, orbgpu.DEPTH_F32) == (0, 1)


# ---------------------------------------------------------------- depth test inputs (checked on the CPU too)

DW, DH, DCAP = 64, 48, 1100
DCOUNTS = np.array([DCAP, 0, 1, 700], np.int32)
DPITCH = DW + 8  # elements
DEPTH_CASES = ["u16_tum", "u16_one", "f32_one", "f32_half"]


def _depth_keypoints():
    """(B, cap) KP_DTYPE: random coordinates inside the map, among them exact
    integers and values just below an integer; the first two keypoints of a
    frame lie outside the map (x = W + 3; y = -2)."""
    rng = np.random.default_rng(77)
    k = np.zeros((len(DCOUNTS), DCAP), orbgpu.KP_DTYPE)
    for b, n in enumerate(DCOUNTS):
        x = rng.uniform(0, DW, n).astype(F32)
        y = rng.uniform(0, DH, n).astype(F32)
        x[x >= DW] = DW - 1  # a float32 rounding of uniform() may reach the open end
        y[y >= DH] = DH - 1
        ix, iy = np.arange(n) % 10 == 3, np.arange(n) % 10 == 5
        x[ix] = np.floor(x[ix])
        y[iy] = np.floor(y[iy])
        jx, jy = np.arange(n) % 10 == 7, np.arange(n) % 10 == 9
        x[jx] = (np.floor(x[jx]) + 1 - rng.uniform(1e-5, 1e-3, jx.sum())).astype(F32)
        y[jy] = (np.floor(y[jy]) + 1 - rng.uniform(1e-5, 1e-3, jy.sum())).astype(F32)
        if n > 0:
            x[0] = DW + 3
        if n > 1:
            y[1] = -2.0
        k["x"][b, :n], k["y"][b, :n] = x, y
        k["octave"][b, :n] = rng.integers(0, 8, n)
    k["size"], k["angle"], k["response"], k["class_id"] = 31.0, 90.0, 12.0, -1
    return k


def _depth_map(case):
    """(maps (B, H, pitch) with pitch > W, depth_factor)"""
    rng = np.random.default_rng(DEPTH_CASES.index(case) + 100)
    B = len(DCOUNTS)
    if case.startswith("u16"):
        m = rng.integers(1, 65536, (B, DH, DPITCH)).astype(np.uint16)
        m[rng.random(m.shape) < 0.25] = 0
        return m, (F32(1.0) / F32(5000.0) if case == "u16_tum" else F32(1.0))
    m = rng.uniform(0.3, 9.0, (B, DH, DPITCH)).astype(F32)
    kind = rng.random(m.shape)
    m[kind < 0.15] = 0.0
    m[(kind >= 0.15) & (kind < 0.3)] *= -1
    m[(kind >= 0.3) & (kind < 0.4)] = np.nan
    m[(kind >= 0.4) & (kind < 0.42)] = -0.0
    return m, F32(1.0 if case == "f32_one" else 0.5)


@pytest.mark.parametrize("case", DEPTH_CASES)
def test_depth_inputs_are_not_vacuous(case):
    """in every frame with >= 100 keypoints between 10 % and 90 % get a depth;
    the special coordinates are present"""
    k = _depth_keypoints()
    m, factor = _depth_map(case)
    for b, n in enumerate(DCOUNTS):
        if n == 0:
            continue
        x, y = k["x"][b, :n], k["y"][b, :n]
        _, d, _ = rgbd_ref.stereo_from_rgbd(m[b, :, :DW], factor, x, y, x, y, K, BF)
        if n >= 100:
            assert 0.1 < (d > 0).mean() < 0.9, (case, b, (d > 0).mean())
            assert (x == np.floor(x)).sum() > 10 and (np.ceil(y) - y < 1e-3).sum() > 10
            assert d[0] == -1 and d[1] == -1
        assert x[0] == DW + 3


# ---------------------------------------------------------------- GPU

def _torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _up16(n):
    return (n + 15) // 16 * 16


@pytest.mark.gpu
def test_gpu_gray_every_rgb_triple():
    """all 2^24 (R, G, B) once in a 4096 x 4096 frame: code RGB, then the same
    triples as BGRA with random alpha, both on the 16-byte path"""
    torch = _torch_gpu()
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v & 255, (v >> 8) & 255, v >> 16], 1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    want = rgbd_ref.gray_from_color(rgb, rgbd_ref.COLOR_RGB)
    assert want.min() == 0 and want.max() == 255
    gray = torch.full((1, 4096, 4096), 0xA5, dtype=torch.uint8, device="cuda")
    orbgpu.gray_from_color_batch(torch.from_numpy(rgb).cuda(), orbgpu.COLOR_RGB, gray)
    assert gray.cpu().numpy().tobytes() == want.tobytes()
    alpha = np.random.default_rng(5).integers(0, 256, (1, 4096, 4096, 1), dtype=np.uint8)
    bgra = np.ascontiguousarray(np.concatenate([rgb[..., ::-1], alpha], 3))
    gray.fill_(0xA5)
    orbgpu.gray_from_color_batch(torch.from_numpy(bgra).cuda(), orbgpu.COLOR_BGRA, gray)
    assert gray.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("code", CODES)
def test_gpu_gray_layouts(code):
    """widths around the 16-pixel chunk x {16-aligned padded pitches and frame
    steps (16-byte path), tightly packed (general path unless the row bytes
    happen to be a multiple of 16), aligned layout from a base pointer off by
    one}: pixels equal the restatement; pad, inter-frame gap and guard-row
    bytes of the destination keep their 0xA5"""
    torch = _torch_gpu()
    ch = rgbd_ref.CHANNELS[code]
    H, B = 5, 3
    rng = np.random.default_rng(code)
    for w in (16, 50, 64, 65, 1241):
        color = rng.integers(0, 256, (B, H, w, ch), dtype=np.uint8)
        want = rgbd_ref.gray_from_color(color, code)
        for layout in ("aligned", "tight", "offset1"):
            if layout == "tight":
                srs, sfs, drs, dfs, soff = w * ch, H * w * ch, w, H * w, 0
            else:
                srs, drs = _up16(w * ch) + 16, _up16(w) + 16
                sfs, dfs, soff = (H + 1) * srs, (H + 2) * drs, (1 if layout == "offset1" else 0)
            src = np.full(soff + B * sfs, 0x3C, np.uint8)
            sv = np.lib.stride_tricks.as_strided(src[soff:], (B, H, w * ch), (sfs, srs, 1))
            sv[...] = color.reshape(B, H, w * ch)
            doff = drs  # one guard row before the first frame, one after the last
            exp = np.full(doff + B * dfs + drs, 0xA5, np.uint8)
            np.lib.stride_tricks.as_strided(exp[doff:], (B, H, w), (dfs, drs, 1))[...] = want
            d_src = torch.from_numpy(src).cuda()
            d_dst = torch.full((len(exp),), 0xA5, dtype=torch.uint8, device="cuda")
            cv = torch.as_strided(d_src, (B, H, w * ch), (sfs, srs, 1), soff)
            gv = torch.as_strided(d_dst, (B, H, w), (dfs, drs, 1), doff)
            if layout != "tight":  # the layouts meant for (and just off) the 16-byte path are what they claim
                assert cv.data_ptr() % 16 == soff and gv.data_ptr() % 16 == 0
            orbgpu.gray_from_color_batch(cv, code, gv, width=w)
            got = d_dst.cpu().numpy()
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (w, layout, len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])
    # (B, H, W, C) form, and the explicit step overrides on a flat buffer
    color = rng.integers(0, 256, (B, H, 32, ch), dtype=np.uint8)
    gray = torch.zeros((B, H, 32), dtype=torch.uint8, device="cuda")
    orbgpu.gray_from_color_batch(torch.from_numpy(color).cuda(), code, gray)
    assert gray.cpu().numpy().tobytes() == rgbd_ref.gray_from_color(color, code).tobytes()
    gray.zero_()
    flat = torch.from_numpy(color.reshape(1, 1, -1)).cuda().expand(B, H, -1)
    orbgpu.gray_from_color_batch(flat, code, gray, width=32, row_step=32 * ch, frame_step=H * 32 * ch)
    assert gray.cpu().numpy().tobytes() == rgbd_ref.gray_from_color(color, code).tobytes()


@pytest.mark.gpu
def test_gpu_gray_more_rows_than_a_grid_dimension():
    """height * batch = 76,800 rows, past the 65,535 limit of gridDim.y / .z"""
    torch = _torch_gpu()
    color = np.random.default_rng(9).integers(0, 256, (256, 300, 16, 3), dtype=np.uint8)
    gray = torch.zeros((256, 300, 16), dtype=torch.uint8, device="cuda")
    orbgpu.gray_from_color_batch(torch.from_numpy(color).cuda(), orbgpu.COLOR_RGB, gray)
    assert gray.cpu().numpy().tobytes() == rgbd_ref.gray_from_color(color, rgbd_ref.COLOR_RGB).tobytes()
    # the same rows off the 16-byte path
    c1 = torch.as_strided(torch.from_numpy(np.concatenate([[0], color.reshape(-1)]).astype(np.uint8)).cuda(),
                          (256, 300, 48), (300 * 48, 48, 1), 1)
    gray.zero_()
    orbgpu.gray_from_color_batch(c1, orbgpu.COLOR_RGB, gray)
    assert gray.cpu().numpy().tobytes() == rgbd_ref.gray_from_color(color, rgbd_ref.COLOR_RGB).tobytes()


SENTINEL = 0x5A5AA5A5


def _sentinel(torch, shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _kps_tensor(torch, host):
    B, cap = host.shape
    return torch.from_numpy(host.view(np.float32).reshape(B, cap, 7).copy()).cuda()


def _kps_host(t):
    B, cap, _ = t.shape
    return t.cpu().numpy().reshape(B, cap * 7).view(orbgpu.KP_DTYPE).reshape(B, cap)


def _check_rgbd_outputs(maps, factor, width, k, ku, counts, uright, depth, x3dc):
    ur, de = uright.cpu().numpy().view(np.uint32), depth.cpu().numpy().view(np.uint32)
    xc = x3dc.cpu().numpy().view(np.uint32) if x3dc is not None else None
    for b, n in enumerate(counts):
        ru, rd, rx = rgbd_ref.stereo_from_rgbd(maps[b, :, :width], factor, k["x"][b, :n], k["y"][b, :n],
                                               ku["x"][b, :n], ku["y"][b, :n], K, BF, want_x3dc=xc is not None)
        assert ur[b, :n].tobytes() == ru.tobytes(), f"frame {b}: mvuRight differs"
        assert de[b, :n].tobytes() == rd.tobytes(), f"frame {b}: mvDepth differs"
        assert (ur[b, n:] == SENTINEL).all() and (de[b, n:] == SENTINEL).all(), f"frame {b}: slots past the count"
        if xc is not None:
            assert xc[b, :n].tobytes() == rx.tobytes(), f"frame {b}: x3Dc differs"
            assert (xc[b, n:] == SENTINEL).all(), f"frame {b}: x3Dc slots past the count"


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEPTH_CASES)
def test_gpu_stereo_from_rgbd(case):
    torch = _torch_gpu()
    cam = orbgpu.Camera.make(*K, TUM1["dist"])
    k = _depth_keypoints()
    maps, factor = _depth_map(case)
    B = len(DCOUNTS)
    kps, cnt = _kps_tensor(torch, k), torch.from_numpy(DCOUNTS).cuda()
    kps_un = torch.zeros_like(kps)
    orbgpu.undistort_keypoints_batch(cam, kps, cnt, kps_un)
    ku = _kps_host(kps_un)
    assert (ku["x"][0] != k["x"][0]).mean() > 0.9  # kpU.x differs from kp.x
    d_maps = torch.from_numpy(maps).cuda()[:, :, :DW]  # padded row step
    if case == "u16_one":
        d_maps = d_maps.view(torch.int16)  # int16 storage is read as uint16
    for with_x3dc in (True, False):
        uright, depth = _sentinel(torch, (B, DCAP)), _sentinel(torch, (B, DCAP))
        x3dc = _sentinel(torch, (B, DCAP, 3)) if with_x3dc else None
        orbgpu.stereo_from_rgbd_batch(d_maps, factor, kps, kps_un, cnt, cam, BF, uright, depth, x3dc)
        _check_rgbd_outputs(maps, factor, DW, k, ku, DCOUNTS, uright, depth, x3dc)


@pytest.mark.gpu
def test_gpu_rgbd_chain_on_one_stream(mono_frames):
    """gray_from_color -> extract_batch -> undistort -> stereo_from_rgbd on one
    non-default stream, synchronised once at the end"""
    torch = _torch_gpu()
    B, H, W = 3, 480, 640
    rng = np.random.default_rng(21)
    rgb = np.clip(mono_frames[:B, :, :, None].astype(np.int16) + rng.integers(-3, 4, (B, H, W, 3)), 0, 255) \
        .astype(np.uint8)
    assert (rgb[..., 0] != rgb[..., 1]).any() and (rgb[..., 1] != rgb[..., 2]).any()
    want_gray = rgbd_ref.gray_from_color(rgb, rgbd_ref.COLOR_RGB)
    dmap = rng.integers(1, 65536, (B, H, W)).astype(np.uint16)
    dmap[rng.random(dmap.shape) < 0.2] = 0
    factor = F32(1.0) / F32(5000.0)
    cam = orbgpu.Camera.make(*K, TUM1["dist"])
    ex = orbgpu.Extractor(max_batch=B)
    cap = ex.max_keypoints

    def outputs():
        return (torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda"),
                torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda"),
                torch.zeros(B, dtype=torch.int32, device="cuda"))

    d_rgb, d_map = torch.from_numpy(rgb).cuda(), torch.from_numpy(dmap).cuda()
    gray = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    kps, desc, counts = outputs()
    kps_un = torch.zeros_like(kps)
    uright, depth = _sentinel(torch, (B, cap)), _sentinel(torch, (B, cap))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    orbgpu.gray_from_color_batch(d_rgb, orbgpu.COLOR_RGB, gray, stream=s)
    ex.extract_batch(gray, kps, desc, counts, stream=s)
    orbgpu.undistort_keypoints_batch(cam, kps, counts, kps_un, stream=s)
    orbgpu.stereo_from_rgbd_batch(d_map, factor, kps, kps_un, counts, cam, BF, uright, depth, stream=s)
    ex.sync(s)
    s.synchronize()
    assert gray.cpu().numpy().tobytes() == want_gray.tobytes()
    # the same extractor on the uploaded restatement-grey frames
    kps2, desc2, counts2 = outputs()
    ex.extract_batch(torch.from_numpy(want_gray).cuda(), kps2, desc2, counts2)
    ex.sync()
    torch.cuda.synchronize()
    n = counts.cpu().numpy()
    assert (n > 100).all() and np.array_equal(n, counts2.cpu().numpy())
    k, k2 = kps.cpu().numpy(), kps2.cpu().numpy()
    d, d2 = desc.cpu().numpy(), desc2.cpu().numpy()
    for b in range(B):
        assert k[b, :n[b]].tobytes() == k2[b, :n[b]].tobytes(), f"frame {b}: keypoints differ"
        assert d[b, :n[b]].tobytes() == d2[b, :n[b]].tobytes(), f"frame {b}: descriptors differ"
    _check_rgbd_outputs(dmap, factor, W, _kps_host(kps), _kps_host(kps_un), n, uright, depth, None)
    valid = depth.cpu().numpy()[0, :n[0]] > 0
    assert 0.5 < valid.mean() < 0.95
