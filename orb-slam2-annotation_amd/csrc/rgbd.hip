// rgbd.hip -- the RGB-D mode's input steps for batches of frames
// (include/orbgpu_rgbd.h): cvtColor(.., CV_*2GRAY) of the colour frames
// (Tracking.cpp:204-225, 250-260, 287-297), and the depth-map scaling
// (Tracking.cpp:264-265) applied at the keypoints inside
// Frame::ComputeStereoFromRGBD (Frame.cpp:751-773), with UnprojectStereo's
// camera-frame point (Frame.cpp:787-794).
//
// Grey: Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (OpenCV 2.4 RGB2Gray<uchar>).
// The 16-byte path gives every lane 16 consecutive pixels of one row: three or
// four 16-byte loads at the lane's own 48- or 64-byte span, one 16-byte store.
// Each 14-bit coefficient is split into its two bytes, so a pixel costs two
// v_dot4_u32_u8 against the pixel's dword (the fourth byte -- alpha, or the
// next pixel's first channel -- meets a zero coefficient):
//   Y = (dot4(p, lo) + 8192 + (dot4(p, hi) << 8)) >> 14, exact in 32 bits.
// The kernel moves whole 16-pixel chunks only; columns past the last whole
// chunk of a row, and every layout that is not 16-byte aligned throughout, go
// through the general kernel (a byte at a time, no alignment assumed).
//
// Depth: one thread per keypoint, blockIdx.y = frame, as undistort_kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/orbgpu_rgbd.h"
#include "host_common.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kCoefR = 4899, kCoefG = 9617, kCoefB = 1868, kRound = 8192;
// grid-stride launches: enough 256-thread blocks to fill 256 CUs at 8 waves per SIMD
constexpr size_t kMaxBlocks = 2048;

__device__ inline uint32_t gray_of(uint32_t px, uint32_t coef_lo, uint32_t coef_hi) {
    const uint32_t lo = __builtin_amdgcn_udot4(px, coef_lo, kRound, false);
    const uint32_t hi = __builtin_amdgcn_udot4(px, coef_hi, 0u, false);
    return (lo + (hi << 8)) >> 14;
}

// bytes [s, s+4) of the little-endian pair (lo, hi), s in 0..3
__device__ inline uint32_t bytes_at(uint32_t lo, uint32_t hi, int s) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
}

// C = 3 or 4 channels.  Chunk t (16 pixels) of the flattened (frame, row, chunk) space.
template <int C>
__global__ __launch_bounds__(kThreads) void gray_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        uint32_t chunks_per_row, uint32_t height, uint32_t total,
                                                        size_t src_row_step, size_t src_frame_step,
                                                        size_t dst_row_step, size_t dst_frame_step, uint32_t coef_lo,
                                                        uint32_t coef_hi) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t t64 = (size_t)blockIdx.x * kThreads + threadIdx.x; t64 < total; t64 += stride) {
        const uint32_t t = (uint32_t)t64;
        const uint32_t row = t / chunks_per_row, chunk = t - row * chunks_per_row;
        const uint32_t frame = row / height, y = row - frame * height;
        const uint4* in = reinterpret_cast<const uint4*>(src + (size_t)frame * src_frame_step +
                                                         (size_t)y * src_row_step + (size_t)chunk * (16 * C));
        uint32_t w[4 * C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uint4 v = in[j];
            w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
        }
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // four pixels -> one output dword
            uint32_t px[4];
            if (C == 4) {
                px[0] = w[4 * q], px[1] = w[4 * q + 1], px[2] = w[4 * q + 2], px[3] = w[4 * q + 3];
            } else {  // 12 bytes in three dwords: pixels at byte 0, 3, 6 and 9
                const uint32_t a = w[3 * q], b = w[3 * q + 1], c = w[3 * q + 2];
                px[0] = a, px[1] = bytes_at(a, b, 3), px[2] = bytes_at(b, c, 2), px[3] = c >> 8;
            }
            uint32_t g[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = gray_of(px[k], coef_lo, coef_hi);
            o[q] = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
        }
        uint4* out = reinterpret_cast<uint4*>(dst + (size_t)frame * dst_frame_step + (size_t)y * dst_row_step +
                                              (size_t)chunk * 16);
        *out = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// Any layout: a block walks rows, its threads the row's pixels.  r_pos / b_pos:
// byte position of R and B inside a pixel.
__global__ void gray_general_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int channels,
                                    int r_pos, int b_pos, int width, int height, size_t rows, size_t src_row_step,
                                    size_t src_frame_step, size_t dst_row_step, size_t dst_frame_step) {
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const size_t frame = row / (size_t)height, y = row - frame * (size_t)height;
        const uint8_t* in = src + frame * src_frame_step + y * src_row_step;
        uint8_t* out = dst + frame * dst_frame_step + y * dst_row_step;
        for (int x = threadIdx.x; x < width; x += blockDim.x) {
            const uint8_t* p = in + (size_t)x * channels;
            out[x] = (uint8_t)(((uint32_t)p[r_pos] * kCoefR + (uint32_t)p[1] * kCoefG + (uint32_t)p[b_pos] * kCoefB +
                                kRound) >> 14);
        }
    }
}

__global__ void rgbd_depth_kernel(const uint8_t* __restrict__ maps, bool is_f32, bool cvt, float factor, int width,
                                  int height, size_t row_step, size_t frame_step,
                                  const orbgpu_keypoint* __restrict__ kps, const orbgpu_keypoint* __restrict__ kps_un,
                                  const int* __restrict__ counts, int cap, float cx, float cy, float invfx,
                                  float invfy, float bf, float* __restrict__ uright, float* __restrict__ depth,
                                  float* __restrict__ x3dc) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= counts[b]) return;
    const size_t slot = (size_t)b * cap + i;
    const float kx = kps[slot].x, ky = kps[slot].y;
    const float ux = kps_un[slot].x, uy = kps_un[slot].y;
    // Mat::at<float>(float, float): the coordinates truncate toward zero
    const int col = (int)kx, row = (int)ky;
    float d = -1.0f;
    if (kx == kx && ky == ky && col >= 0 && col < width && row >= 0 && row < height) {
        const uint8_t* p = maps + (size_t)b * frame_step + (size_t)row * row_step;
        const float s = is_f32 ? reinterpret_cast<const float*>(p)[col]
                               : (float)reinterpret_cast<const uint16_t*>(p)[col];
        d = cvt ? __fadd_rn(__fmul_rn(s, factor), 0.0f) : s;
    }
    const bool valid = d > 0.0f;  // false for NaN
    depth[slot] = valid ? d : -1.0f;
    uright[slot] = valid ? __fsub_rn(ux, __fdiv_rn(bf, d)) : -1.0f;
    if (x3dc) {
        float* o = x3dc + slot * 3;
        o[0] = valid ? __fmul_rn(__fmul_rn(__fsub_rn(ux, cx), d), invfx) : 0.0f;
        o[1] = valid ? __fmul_rn(__fmul_rn(__fsub_rn(uy, cy), d), invfy) : 0.0f;
        o[2] = valid ? d : 0.0f;
    }
}

inline bool aligned16(uintptr_t v) { return (v & 15) == 0; }

}  // namespace

extern "C" int orbgpu_gray_from_color_batch_device(const uint8_t* d_color, int code, int width, int height, int batch,
                                                   size_t src_row_step, size_t src_frame_step, uint8_t* d_gray,
                                                   size_t dst_row_step, size_t dst_frame_step, void* stream) {
    if (!d_color || !d_gray || width <= 0 || height <= 0 || batch < 0 || code < ORBGPU_COLOR_RGB ||
        code > ORBGPU_COLOR_BGRA)
        return orbgpu::fail(ORBGPU_ERR_ARG, "invalid argument");
    const int channels = code >= ORBGPU_COLOR_RGBA ? 4 : 3;
    if (src_row_step < (size_t)width * channels || dst_row_step < (size_t)width)
        return orbgpu::fail(ORBGPU_ERR_ARG, "row step shorter than a row");
    if (batch > 1 && (src_frame_step < src_row_step * height || dst_frame_step < dst_row_step * height))
        return orbgpu::fail(ORBGPU_ERR_ARG, "frame step shorter than a frame");
    if (batch == 0) return ORBGPU_OK;
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool bgr = code == ORBGPU_COLOR_BGR || code == ORBGPU_COLOR_BGRA;
    const int r_pos = bgr ? 2 : 0, b_pos = bgr ? 0 : 2;
    const size_t rows = (size_t)height * batch;

    const bool fast = aligned16((uintptr_t)d_color) && aligned16((uintptr_t)d_gray) && aligned16(src_row_step) &&
                      aligned16(dst_row_step) &&
                      (batch == 1 || (aligned16(src_frame_step) && aligned16(dst_frame_step)));
    int done = 0;  // columns the 16-byte kernel covers
    if (fast && width >= 16) {
        const size_t chunks_per_row = (size_t)width / 16, total = rows * chunks_per_row;
        if (total > 0xFFFFFFFFull) return orbgpu::fail(ORBGPU_ERR_UNSUPPORTED, "more than 2^32 16-pixel chunks");
        const uint32_t c0 = bgr ? kCoefB : kCoefR, c2 = bgr ? kCoefR : kCoefB;
        const uint32_t lo = (c0 & 255) | ((kCoefG & 255) << 8) | ((c2 & 255) << 16);
        const uint32_t hi = (c0 >> 8) | ((kCoefG >> 8) << 8) | ((c2 >> 8) << 16);
        const dim3 grid((unsigned)std::min((total + kThreads - 1) / kThreads, kMaxBlocks));
        if (channels == 3)
            hipLaunchKernelGGL(gray_kernel<3>, grid, dim3(kThreads), 0, s, d_color, d_gray, (uint32_t)chunks_per_row,
                               (uint32_t)height, (uint32_t)total, src_row_step, src_frame_step, dst_row_step,
                               dst_frame_step, lo, hi);
        else
            hipLaunchKernelGGL(gray_kernel<4>, grid, dim3(kThreads), 0, s, d_color, d_gray, (uint32_t)chunks_per_row,
                               (uint32_t)height, (uint32_t)total, src_row_step, src_frame_step, dst_row_step,
                               dst_frame_step, lo, hi);
        ORB_HIP(hipGetLastError());
        done = width / 16 * 16;
    }
    if (done < width) {
        const int rest = width - done;
        const int threads = rest <= 64 ? 64 : kThreads;
        // a wide row keeps a block busy; narrow rows want more blocks in flight
        const dim3 grid((unsigned)std::min(rows, kMaxBlocks * (size_t)(kThreads / threads) * 4));
        hipLaunchKernelGGL(gray_general_kernel, grid, dim3(threads), 0, s, d_color + (size_t)done * channels,
                           d_gray + done, channels, r_pos, b_pos, rest, height, rows, src_row_step, src_frame_step,
                           dst_row_step, dst_frame_step);
        ORB_HIP(hipGetLastError());
    }
    return ORBGPU_OK;
}

extern "C" int orbgpu_stereo_from_rgbd_batch_device(const void* d_depth_maps, int depth_type, float depth_factor,
                                                    int width, int height, size_t row_step, size_t frame_step,
                                                    int batch, const orbgpu_keypoint* d_kps,
                                                    const orbgpu_keypoint* d_kps_un, const int* d_counts,
                                                    int kp_capacity, const orbgpu_camera* cam, float bf,
                                                    float* d_uright, float* d_depth, float* d_x3dc, void* stream) {
    if (!d_depth_maps || !d_kps || !d_kps_un || !d_counts || !cam || !d_uright || !d_depth || width <= 0 ||
        height <= 0 || batch < 0 || kp_capacity <= 0 ||
        (depth_type != ORBGPU_DEPTH_U16 && depth_type != ORBGPU_DEPTH_F32))
        return orbgpu::fail(ORBGPU_ERR_ARG, "invalid argument");
    const bool is_f32 = depth_type == ORBGPU_DEPTH_F32;
    const size_t elem = is_f32 ? sizeof(float) : sizeof(uint16_t);
    if (row_step < (size_t)width * elem || row_step % elem || ((uintptr_t)d_depth_maps % elem) ||
        (batch > 1 && (frame_step < row_step * height || frame_step % elem)))
        return orbgpu::fail(ORBGPU_ERR_ARG, "depth maps: steps shorter than a row / a frame, or not element-aligned");
    if (batch == 0) return ORBGPU_OK;
    if (batch > 65535) return orbgpu::fail(ORBGPU_ERR_UNSUPPORTED, "batch > 65535");
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    const bool cvt = !is_f32 || std::fabs(depth_factor - 1.0f) > 1e-5f;  // Tracking.cpp:264
    const float invfx = 1.0f / cam->fx, invfy = 1.0f / cam->fy;           // Frame.cpp:172-173
    hipLaunchKernelGGL(rgbd_depth_kernel, dim3((kp_capacity + 255) / 256, batch), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t*>(d_depth_maps), is_f32, cvt,
                       depth_factor, width, height, row_step, frame_step, d_kps, d_kps_un, d_counts, kp_capacity,
                       cam->cx, cam->cy, invfx, invfy, bf, d_uright, d_depth, d_x3dc);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}
