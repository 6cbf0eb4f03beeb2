// loop_device.h -- what the two round-robin RANSAC kernels of
// LoopClosing::ComputeSim3 share (loop.hip: compute_sim3_kernel, one call to
// the first return; loop_verify.hip: the resumable kernel of the verified
// loop): the Sim3Solver workspace layout, the glibc stream step,
// SetRansacParameters, one hypothesis' three swap-remove draws and the scoring
// of a pair of hypotheses by a wave.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/orbgpu_loop.h"
#include "ransac_device.h"
#include "sim3_device.h"

namespace orbgpu {
namespace loopdev {

using namespace sim3dev;
using namespace ransacdev;

#ifndef ORBGPU_SIM3_THREADS
#define ORBGPU_SIM3_THREADS 512
#endif
constexpr int kQThreads = ORBGPU_SIM3_THREADS;  // 8 scoring waves, 2 per SIMD
constexpr int kWin = 256;  // hypotheses solved and scored per window
constexpr int kMaxC = ORBGPU_LOOP_MAX_CANDIDATES;

struct Workspace {  // SoA, candidate c at c * stride
    float* X1;      // 3 per correspondence
    float* X2;
    float* e1;
    float* e2;
    int* idx1;
    float2* P1;     // mvP1im1 / mvP2im2: FromCameraToImage of X1 / X2 (the ctor's, Sim3Solver.cpp:97-98)
    float2* P2;
};

__host__ __device__ inline Workspace carve(void* base, int n_cand, int stride) {
    const size_t n = (size_t)n_cand * stride;
    char* p = static_cast<char*>(base);
    Workspace w;
    w.X1 = reinterpret_cast<float*>(p);
    p += align256(n * 12);
    w.X2 = reinterpret_cast<float*>(p);
    p += align256(n * 12);
    w.e1 = reinterpret_cast<float*>(p);
    p += align256(n * 4);
    w.e2 = reinterpret_cast<float*>(p);
    p += align256(n * 4);
    w.idx1 = reinterpret_cast<int*>(p);
    p += align256(n * 4);
    w.P1 = reinterpret_cast<float2*>(p);
    p += align256(n * 8);
    w.P2 = reinterpret_cast<float2*>(p);
    return w;
}

inline size_t workspace_bytes(int n_cand, int stride) {
    const size_t n = (size_t)(n_cand > 0 ? n_cand : 1) * (stride > 0 ? stride : 1);
    return 2 * align256(n * 12) + 3 * align256(n * 4) + 2 * align256(n * 8);
}

// Sim3Solver::SetRansacParameters (Sim3Solver.cpp:111-141): mRansacMaxIts of a solver with N
// correspondences (0 for N < 0, no solver)
__device__ inline int ransac_max_iterations(int N, const orbgpu_sim3_ransac_params& prm) {
    int max_its = 0;
    if (N >= 0) {
        const float eps = (float)prm.min_inliers / (float)N;
        int n_it;
        if (prm.min_inliers == N) {
            n_it = 1;
        } else {
            n_it = ransac_iterations(prm.probability, eps);
        }
        max_its = max(1, min(n_it, prm.max_iterations));
    }
    return max_its;
}

// one hypothesis' minimal set (Sim3Solver.cpp:172-183): three swap-remove draws
__device__ __forceinline__ void draw_triplet(int N, int32_t* s_r, int& rf, int& rb, int32_t* gen, int* trip) {
    draw_set<3>(N, s_r, rf, rb, gen, trip);
}

// CheckInliers of hypothesis H (and Hb when two) over one candidate's N correspondences at
// offset o, by one wave: one pass tests both (each correspondence loaded once).  Four
// correspondences per lane in flight (one wave per SIMD here: the test's loads and FP64 chains are
// latency bound, so independent work is what hides them); indices past N are clamped and masked.
__device__ __forceinline__ void score_pair(const Workspace& ws, size_t o, int N, const float* K1, const float* K2,
                                           const Hyp& H, const Hyp& Hb, bool two, int lane, int& cnt_out,
                                           int& cntb_out) {
    int cnt = 0, cntb = 0;
    for (int i0 = lane; i0 < N; i0 += 256) {
        bool in[4], inb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(i0 + 64 * u, N - 1);
            const float* X1 = ws.X1 + 3 * (o + i);
            const float* X2 = ws.X2 + 3 * (o + i);
            const float2 p1 = ws.P1[o + i], p2 = ws.P2[o + i];
            const float e1 = ws.e1[o + i], e2 = ws.e2[o + i];
            in[u] = is_inlier_pre(H, K1, K2, X1, X2, p1, p2, e1, e2);
            inb[u] = two && is_inlier_pre(Hb, K1, K2, X1, X2, p1, p2, e1, e2);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = i0 + 64 * u < N;
            cnt += __popcll(__ballot(in[u] && live));
            if (two) cntb += __popcll(__ballot(inb[u] && live));
        }
    }
    cnt_out = cnt;
    cntb_out = cntb;
}

}  // namespace loopdev
}  // namespace orbgpu
