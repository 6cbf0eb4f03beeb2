// match.cpp -- host entry points of match.hip and pack.hip (include/orbgpu.h):
// ORBmatcher::SearchForInitialization in its device, stream and host forms,
// Hamming distances of descriptor pairs, row packing.
#include <algorithm>

#include "../../include/orbgpu.h"
#include "host_common.h"
#include "host_ctx.h"
#include "orbgpu_kernels.h"

using namespace orbgpu;

extern "C" {

int orbgpu_hamming_pairs_device(const uint8_t* a, const uint8_t* b, int n, int* dist, void* stream) {
    if (n < 0 || (n > 0 && (!a || !b || !dist))) return fail(ORBGPU_ERR_ARG, "invalid argument");
    if (((uintptr_t)a | (uintptr_t)b) & 31) return fail(ORBGPU_ERR_ARG, "descriptors must be 32-byte aligned");
    ORB_HIP(launch_hamming_pairs(a, b, n, dist, (hipStream_t)stream));
    return ORBGPU_OK;
}

int orbgpu_pack_rows_device(int batch, int cap, int ntensors, const orbgpu_pack_desc* d, void* stream) {
    if (batch < 0 || cap < 0 || ntensors < 0 || ntensors > 4 || (ntensors > 0 && !d))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    for (int t = 0; t < ntensors; ++t)
        if (!d[t].rows || !d[t].packed || !d[t].counts || d[t].row_bytes <= 0 || (d[t].row_bytes & 3) ||
            (((uintptr_t)d[t].rows | (uintptr_t)d[t].packed) & 3))
            return fail(ORBGPU_ERR_ARG, "pack: rows must be 4-byte multiples at 4-byte aligned addresses");
    ORB_HIP(launch_pack_rows(batch, cap, ntensors, d, (hipStream_t)stream));
    return ORBGPU_OK;
}

int orbgpu_search_for_initialization_batch_device_bounded(
    int batch, orbgpu_grid_bounds bd, const orbgpu_keypoint* kps1, const uint8_t* desc1, const int* n1, size_t stride1,
    const orbgpu_keypoint* kps2, const uint8_t* desc2, const int* n2, size_t stride2, float* prev_xy, int window,
    float nnratio, int flags, int max_level0, int* matches12, int* nmatches, void* stream) {
    if (batch <= 0 || !kps1 || !kps2 || !desc1 || !desc2 || !n1 || !n2 || !matches12 || !nmatches ||
        !(bd.max_x > bd.min_x) || !(bd.max_y > bd.min_y) || max_level0 < 0)
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    ORB_HIP(launch_match_init(batch, bd.min_x, bd.max_x, bd.min_y, bd.max_y, kps1, desc1, n1, stride1, kps2, desc2, n2, stride2, prev_xy,
                              window, nnratio, flags, matches12, nmatches, (hipStream_t)stream, (size_t)max_level0));
    return ORBGPU_OK;
}

int orbgpu_search_for_initialization_stream_device(int batch, orbgpu_grid_bounds bd, const orbgpu_keypoint* kps,
                                                   const uint8_t* desc, const int* n, size_t stride,
                                                   const orbgpu_keypoint* prev_kps, const uint8_t* prev_desc,
                                                   const int* prev_n, float* prev_xy, int window, float nnratio,
                                                   int flags, int max_level0, int* matches12, int* nmatches,
                                                   void* stream) {
    if (batch <= 0 || !kps || !desc || !n || !prev_kps || !prev_desc || !prev_n || !matches12 || !nmatches ||
        stride == 0 || !(bd.max_x > bd.min_x) || !(bd.max_y > bd.min_y) || max_level0 < 0)
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    MatchFirstF1 first;
    first.kps = prev_kps;
    first.desc = prev_desc;
    first.n = prev_n;
    ORB_HIP(launch_match_init(batch, bd.min_x, bd.max_x, bd.min_y, bd.max_y, kps, desc, n, stride, kps, desc, n,
                              stride, prev_xy, window, nnratio, flags, matches12, nmatches, (hipStream_t)stream,
                              (size_t)max_level0, first));
    return ORBGPU_OK;
}

int orbgpu_search_for_initialization_batch_device(int batch, orbgpu_grid_bounds bd, const orbgpu_keypoint* kps1,
                                                  const uint8_t* desc1, const int* n1, size_t stride1,
                                                  const orbgpu_keypoint* kps2, const uint8_t* desc2, const int* n2,
                                                  size_t stride2, float* prev_xy, int window, float nnratio,
                                                  int flags, int* matches12, int* nmatches, void* stream) {
    return orbgpu_search_for_initialization_batch_device_bounded(batch, bd, kps1, desc1, n1, stride1, kps2, desc2, n2,
                                                                 stride2, prev_xy, window, nnratio, flags, 0,
                                                                 matches12, nmatches, stream);
}

int orbgpu_search_for_initialization(orbgpu_grid_bounds bd, const orbgpu_keypoint* kps1, const uint8_t* desc1,
                                     int n1, const orbgpu_keypoint* kps2, const uint8_t* desc2, int n2,
                                     float* prev_xy, int window, float nnratio, int flags, int* matches12,
                                     int* nmatches) {
    if (n1 < 0 || n2 < 0 || !matches12 || !nmatches) return fail(ORBGPU_ERR_ARG, "invalid argument");
    int rc = check_device();
    if (rc) return rc;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    const size_t n1c = std::max(n1, 1), n2c = std::max(n2, 1);
    const int ns[3] = {n1, n2, 0};
    const orbgpu_keypoint *dk1, *dk2;
    const uint8_t *dd1, *dd2;
    int *dn, *dm;
    float* dp;
    HostCall call(*ctx);
    rc = call.run([&](HostCall& A) {
        dk1 = A.inout(kps1, (size_t)n1, n1c);
        dk2 = A.inout(kps2, (size_t)n2, n2c);
        dd1 = A.inout(desc1, 32 * (size_t)n1, 32 * n1c);
        dd2 = A.inout(desc2, 32 * (size_t)n2, 32 * n2c);
        dn = A.inout(ns, 3);
        dm = A.out<int>(n1c);
        dp = prev_xy ? A.inout(prev_xy, 2 * (size_t)n1, 2 * n1c) : nullptr;
    });
    if (rc) return rc;
    // the number of level-0 keypoints bounds which matcher variants can be
    // needed, so a 1000-feature frame (~220 at level 0) takes one launch, not
    // one per variant (all octave-0 entries are counted: an upper bound of the
    // leading run the kernel uses, whatever the order)
    auto level0 = [](const orbgpu_keypoint* k, int n) {
        int c = 0;
        for (int i = 0; i < n; ++i) c += k[i].octave == 0;
        return c;
    };
    const size_t n0 = (size_t)std::max(std::max(level0(kps1, n1), level0(kps2, n2)), 1);
    if (!(bd.max_x > bd.min_x) || !(bd.max_y > bd.min_y)) return fail(ORBGPU_ERR_ARG, "invalid argument");
    ORB_HIP(launch_match_init(1, bd.min_x, bd.max_x, bd.min_y, bd.max_y, dk1, dd1, dn, n1c, dk2, dd2, dn + 1, n2c, dp,
                              window, nnratio, flags, dm, dn + 2, ctx->stream, n0));
    call.fetch(dm, matches12, (size_t)n1 * sizeof(int));
    call.fetch(dn + 2, nmatches, sizeof(int));
    if (prev_xy) call.fetch(dp, prev_xy, (size_t)n1 * 2 * sizeof(float));
    if ((rc = call.finish())) return rc;
    if (*nmatches < 0) {
        *nmatches = 0;
        return fail(ORBGPU_ERR_CAPACITY, "matcher: more than 2048 level-0 keypoints in a frame");
    }
    return ORBGPU_OK;
}

}  // extern "C"
