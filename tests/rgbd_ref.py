"""numpy restatement of the RGB-D input steps (include/orbgpu_rgbd.h):

* gray_from_color: cvtColor(.., CV_{RGB,BGR,RGBA,BGRA}2GRAY) of OpenCV 2.4
  (RGB2Gray<uchar>: Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14, alpha ignored).
* stereo_from_rgbd: imDepth.convertTo(CV_32F, mDepthMapFactor)
  (Tracking.cpp:264-265) sampled at the keypoints, Frame::ComputeStereoFromRGBD
  (Frame.cpp:751-773) and Frame::UnprojectStereo's x3Dc (Frame.cpp:787-794).

Every float operation is a single np.float32 operation; the sample index is
the truncated (astype(np.int64)) raw keypoint coordinate.
"""
import numpy as np

COLOR_RGB, COLOR_BGR, COLOR_RGBA, COLOR_BGRA = 0, 1, 2, 3
CHANNELS = {COLOR_RGB: 3, COLOR_BGR: 3, COLOR_RGBA: 4, COLOR_BGRA: 4}
F32 = np.float32


def gray_from_color(color: np.ndarray, code: int) -> np.ndarray:
    """color: uint8 (..., C) -> uint8 (...)"""
    color = np.asarray(color, np.uint8)
    assert color.shape[-1] == CHANNELS[code]
    r_pos, b_pos = (2, 0) if code in (COLOR_BGR, COLOR_BGRA) else (0, 2)
    r = color[..., r_pos].astype(np.uint32)
    g = color[..., 1].astype(np.uint32)
    b = color[..., b_pos].astype(np.uint32)
    return ((r * np.uint32(4899) + g * np.uint32(9617) + b * np.uint32(1868) + np.uint32(8192)) >> np.uint32(14)) \
        .astype(np.uint8)


def stereo_from_rgbd(depth_map: np.ndarray, depth_factor, kx, ky, ux, uy, cam, bf, want_x3dc=True):
    """One frame.  depth_map: (H, W) uint16 or float32; kx, ky: raw keypoint
    coordinates, ux, uy: undistorted ones (float32 arrays of one length);
    cam = (fx, fy, cx, cy).  -> uright, depth (float32 (N,)), x3dc (float32
    (N, 3)) or None."""
    assert depth_map.dtype in (np.uint16, np.float32)
    factor = F32(depth_factor)
    cvt = depth_map.dtype != np.float32 or np.abs(factor - F32(1.0)) > F32(1e-5)
    kx, ky, ux, uy = (np.asarray(a, F32) for a in (kx, ky, ux, uy))
    h, w = depth_map.shape
    with np.errstate(invalid="ignore"):
        col, row = kx.astype(np.int64), ky.astype(np.int64)  # truncation toward zero
    inside = (col >= 0) & (col < w) & (row >= 0) & (row < h) & ~np.isnan(kx) & ~np.isnan(ky)
    s = depth_map[np.where(inside, row, 0), np.where(inside, col, 0)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = (s.astype(F32) * factor + F32(0.0)).astype(F32) if cvt else s.astype(F32)
        d = np.where(inside, d, F32(-1.0)).astype(F32)
        valid = d > F32(0.0)  # false for NaN
        dv = np.where(valid, d, F32(1.0)).astype(F32)
        depth = np.where(valid, d, F32(-1.0)).astype(F32)
        uright = np.where(valid, ux - (F32(bf) / dv).astype(F32), F32(-1.0)).astype(F32)
        x3dc = None
        if want_x3dc:
            fx, fy, cx, cy = (F32(v) for v in cam)
            invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
            x = (((ux - cx).astype(F32) * dv).astype(F32) * invfx).astype(F32)
            y = (((uy - cy).astype(F32) * dv).astype(F32) * invfy).astype(F32)
            x3dc = np.where(valid[:, None], np.stack([x, y, dv], 1), F32(0.0)).astype(F32)
    return uright, depth, x3dc
