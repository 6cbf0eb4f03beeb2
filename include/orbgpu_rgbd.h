/*
 * orbgpu_rgbd.h -- the RGB-D sensor mode's input steps, batched on the GPU
 * (conventions as orbgpu_frame.h):
 *   cvtColor(.., CV_{RGB,BGR,RGBA,BGRA}2GRAY)  src/Tracking.cpp:204-225, 250-260, 287-297
 *   imDepth.convertTo(CV_32F, mDepthMapFactor) src/Tracking.cpp:264-265
 *   Frame::ComputeStereoFromRGBD               src/Frame.cpp:751-773
 *   Frame::UnprojectStereo (x3Dc only)         src/Frame.cpp:787-794, 172-173
 * The grey arithmetic is OpenCV 2.4's RGB2Gray<uchar> as recalled
 * (modules/imgproc/src/color.cpp): Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14
 * in 32-bit integers, alpha ignored; the depth scaling is its
 * cvtScale_<ushort|float, float, float>.  Parity against a real OpenCV build
 * is unpinned, like the other OpenCV-derived stages.
 *
 * Only the batched device form exists: the per-call RGB-D Frame constructor
 * works unchanged with the drop-in ORBextractor.
 */
#ifndef ORBGPU_RGBD_H
#define ORBGPU_RGBD_H

#include "orbgpu_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ORBGPU_COLOR_RGB = 0, ORBGPU_COLOR_BGR = 1, ORBGPU_COLOR_RGBA = 2, ORBGPU_COLOR_BGRA = 3 };
enum { ORBGPU_DEPTH_U16 = 0, ORBGPU_DEPTH_F32 = 1 };

/* cvtColor(.., CV_{RGB,BGR,RGBA,BGRA}2GRAY) of OpenCV 2.4 for `batch`
 * interleaved 8-bit frames: pixel (x, y) of frame b is the 3 or 4 bytes at
 * d_color + b*src_frame_step + y*src_row_step + x*channels, its grey value the
 * byte at d_gray + b*dst_frame_step + y*dst_row_step + x.  Bytes of a
 * destination row from `width` to dst_row_step are not written.  Source and
 * destination must not overlap (not checked).
 * When both pointers and all four steps are multiples of 16 the 16-byte path
 * runs (frame steps are not looked at for batch == 1); any other layout takes
 * the general path, chosen per call.  A destination with a 16-byte-aligned
 * base and dst_row_step % 16 == 0 is what orbgpu_extract_batch_device takes.
 * ORBGPU_ERR_ARG: a NULL pointer, width/height <= 0, batch < 0, an unknown
 * code, a row step shorter than a row, or (batch > 1) a frame step shorter
 * than a frame; these are checked before the device is. */
int orbgpu_gray_from_color_batch_device(const uint8_t* d_color, int code, int width, int height, int batch,
                                        size_t src_row_step, size_t src_frame_step, uint8_t* d_gray,
                                        size_t dst_row_step, size_t dst_frame_step, void* stream);

/* mvuRight / mvDepth of `batch` RGB-D frames of one camera.  Depth map b is
 * at d_depth_maps + b*frame_step, row y at + y*row_step (bytes), elements
 * uint16 or float by depth_type.  depth_factor is mDepthMapFactor after the
 * reference's inversion (Tracking.cpp:168-172; TUM: 1.0f/5000.0f).
 *   cvt = depth_type != F32 || fabsf(depth_factor - 1.0f) > 1e-5f      (Tracking.cpp:264)
 *   s   = map[(int)kp.y][(int)kp.x] of the raw keypoint (truncation toward zero)
 *   d   = cvt ? (float)s * depth_factor + 0.0f : s
 *   d > 0:  depth = d, uright = kpU.x - bf / d;  otherwise (0, negative, NaN) both -1.
 * A truncated index outside [0,width) x [0,height), or a NaN coordinate, is
 * an out-of-bounds read in the reference; here it yields -1.
 * d_x3dc (may be NULL): Frame::UnprojectStereo's camera-frame point, 3 floats
 * at (b*kp_capacity + i)*3: x = (kpU.x - cx) * z * invfx, y = (kpU.y - cy) * z
 * * invfy, z, in float, left to right, invfx = 1.0f / fx; three zeros for an
 * invalid point.  The world transform (mRwc * x3Dc + mOw) is the caller's.
 * Slots i >= d_counts[b] are not written.  Argument checks as above. */
int orbgpu_stereo_from_rgbd_batch_device(const void* d_depth_maps, int depth_type, float depth_factor, int width,
                                         int height, size_t row_step, size_t frame_step, int batch,
                                         const orbgpu_keypoint* d_kps, const orbgpu_keypoint* d_kps_un,
                                         const int* d_counts, int kp_capacity, const orbgpu_camera* cam, float bf,
                                         float* d_uright, float* d_depth, float* d_x3dc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
