// ransac_device.h -- what the device-resident RANSAC loops share (loop.hip,
// loop_verify.hip: LoopClosing::ComputeSim3; reloc.hip: Tracking::Relocalization):
// the glibc stream step, RandomInt, the swap-remove draw of a minimal set, the
// iteration bound of SetRansacParameters, the order-preserving compaction of a
// block's stripe, the carving of an opaque state block and the projection
// call of an idle query.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/orbgpu_proj.h"

namespace orbgpu {
namespace ransacdev {

__host__ __device__ inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// the next array of an opaque block: `count` items, 256-byte aligned
template <class T>
__host__ __device__ inline T* take(char*& p, size_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += align256(count * sizeof(T));
    return r;
}

// the same on an address kept as an integer: a size query carves from a null base, and pointer
// arithmetic on a null pointer is undefined
template <class T>
__host__ __device__ inline T* take(uintptr_t& p, size_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += align256(count * sizeof(T));
    return r;
}

// glibc random_r TYPE_3 step (csrc/ransac.cpp restates the same generator):
// returns the raw sum written into the state; rand() is raw >> 1
__device__ inline uint32_t rand_next_raw(int32_t* r, int& f, int& b) {
    const uint32_t val = (uint32_t)r[f] + (uint32_t)r[b];
    r[f] = (int32_t)val;
    if (++f >= 31) {
        f = 0;
        ++b;
    } else if (++b >= 31) {
        b = 0;
    }
    return val;
}

// DUtils::Random::RandomInt(0, d-1)
__device__ inline int random_below(int32_t v, int d) {
    return (int)(((double)v / ((double)2147483647 + 1.0)) * d);
}

// ceil(log(1 - p) / log(1 - eps^3)) as an int, the way x86 converts it: the iteration count of
// Sim3Solver::SetRansacParameters (Sim3Solver.cpp:135) and PnPsolver::SetRansacParameters
// (PnPsolver.cpp:188), whose pow(float, int) is the double pow
__device__ inline int ransac_iterations(double probability, float eps) {
    const double v = ceil(log(1.0 - probability) / log(1.0 - pow((double)eps, 3.0)));
    // an out-of-range double -> int conversion is INT_MIN on x86 (cvttsd2si)
    return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (int)0x80000000;
}

// one hypothesis' minimal set: vAvailableIndices = mvAllIndices; K x RandomInt + swap-remove
// (Sim3Solver.cpp:172-183, K = 3; PnPsolver.cpp:230-244, K = 4) over N correspondences.
// gen[0..K-1] = the raw values drawn.
template <int K>
__device__ __forceinline__ void draw_set(int N, int32_t* s_r, int& rf, int& rb, int32_t* gen, int* set) {
    int pos[K - 1], val[K - 1], nmod = 0;
    for (int d = 0; d < K; ++d) {
        const int size = N - d;
        const uint32_t raw = rand_next_raw(s_r, rf, rb);
        gen[d] = (int32_t)raw;
        const int r = random_below((int32_t)(raw >> 1), size);
        int idx = r;  // vAvailableIndices[r] after the earlier swaps
        for (int m = nmod - 1; m >= 0; --m)
            if (pos[m] == r) {
                idx = val[m];
                break;
            }
        int back = size - 1;  // vAvailableIndices.back()
        for (int m = nmod - 1; m >= 0; --m)
            if (pos[m] == size - 1) {
                back = val[m];
                break;
            }
        set[d] = idx;
        if (d < K - 1) {
            pos[nmod] = r;
            val[nmod] = back;
            ++nmod;
        }
    }
}

// Order-preserving compaction of a block, one stripe of blockDim.x items at a time:
// compact_slot is the output index of this thread's item (meaningful when ok) given `base` items
// before the stripe; compact_advance then moves base past the stripe.  Every thread of the block
// calls both; s_wave holds one int per wave and the caller puts a __syncthreads() between two
// stripes.
__device__ __forceinline__ int compact_slot(bool ok, int lane, int wave, int* s_wave, int base) {
    const unsigned long long m = __ballot(ok);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = base;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    return before + (int)__popcll(m & ((1ull << lane) - 1));
}
template <int kThreads>
__device__ __forceinline__ void compact_advance(const int* s_wave, int& base) {
    for (int w = 0; w < kThreads / 64; ++w) base += s_wave[w];
}

// an idle query's projection call: no keypoints, no points (proj_kernel then writes only its count)
__device__ inline void idle_call(orbgpu_proj_call& c, int variant) {
    int* w = reinterpret_cast<int*>(&c);
    for (int k = 0; k < (int)(sizeof(orbgpu_proj_call) / 4); ++k) w[k] = 0;
    c.variant = variant;
    c.target.n_levels = 1;
    c.target.max_x = 1.f;
    c.target.max_y = 1.f;
}

}  // namespace ransacdev
}  // namespace orbgpu
