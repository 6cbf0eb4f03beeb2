// stereo.cpp -- host entry points of stereo.hip (include/orbgpu_stereo.h):
// Frame::ComputeStereoMatches over an extractor's last batch, or over the last
// single frames of two extractors.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "../../include/orbgpu_stereo.h"
#include "extractor.h"
#include "host_ctx.h"
#include "stereo_kernels.h"

using namespace orbgpu;

namespace {

// StereoArgs common to both entry points: level sizes and scales, thresholds,
// and the level bases of the left / right image of pair 0 (lb0 / rb0: level 0
// from the caller's image pointers, levels >= 1 from the extractors' pyramids)
void stereo_args(const orbgpu_extractor* left, const orbgpu_extractor* right, int lframe, int rframe,
                 const uint8_t* l0, const uint8_t* r0, size_t row_step, size_t pair_step0, int cap, float bf,
                 float min_z, StereoArgs& a) {
    const Geom& g = left->geo.g;
    std::memset(&a, 0, sizeof(a));
    for (int l = 0; l < g.nlevels; ++l) {
        if (l == 0) {
            a.lvl_base[0] = l0;
            a.lvl_base_r[0] = r0;
            a.lvl_pair[0] = pair_step0;
            a.lvl_pitch[0] = (int)row_step;
        } else {
            a.lvl_base[l] = left->d_pyr + g.lv[l].offset + (size_t)lframe * g.lv[l].frame_bytes;
            a.lvl_base_r[l] = right->d_pyr + g.lv[l].offset + (size_t)rframe * g.lv[l].frame_bytes;
            a.lvl_pair[l] = 2 * g.lv[l].frame_bytes;
            a.lvl_pitch[l] = g.lv[l].pitch;
        }
        a.lvl_w[l] = g.lv[l].w;
        a.lvl_h[l] = g.lv[l].h;
        a.scale[l] = left->geo.scale[l];
        a.inv_scale[l] = left->geo.inv_scale[l];
    }
    a.cap = cap;
    a.bf = bf;
    a.max_d = bf / min_z;  // +inf for min_z = 0, as the reference (Frame.cpp:581)
    a.th_orb = (100 + 50) / 2;
    a.rr = (int)std::ceil(2.0f * left->geo.scale[g.nlevels - 1]) + 1;
}

}  // namespace

extern "C" {

// Frame::ComputeStereoMatches (Frame.cpp:540-748) over the last extraction.
int orbgpu_stereo_matches_batch_device(orbgpu_extractor* e, const uint8_t* d_images, size_t row_step,
                                       size_t frame_step, int npairs, const orbgpu_keypoint* d_kps,
                                       const uint8_t* d_desc, const int* d_counts, int kp_capacity, float bf,
                                       float min_z, float* d_uright, float* d_depth, void* stream) {
    if (!e || !d_images || !d_kps || !d_desc || !d_counts || !d_uright || !d_depth)
        return fail(ORBGPU_ERR_ARG, "NULL argument");
    DeviceScope ds_(e->device);
    if (npairs < 0 || 2 * npairs > e->p.max_batch) return fail(ORBGPU_ERR_ARG, "npairs exceeds max_batch / 2");
    if (kp_capacity < e->geo.max_kps || kp_capacity > 65535)
        return fail(ORBGPU_ERR_ARG, "kp_capacity must be >= max_keypoints and < 65536");
    const Geom& g = e->geo.g;
    if (stereo_lds_bytes(kp_capacity, g.lv[0].h) > 160 * 1024)
        return fail(ORBGPU_ERR_UNSUPPORTED, "stereo LDS tables exceed 160 KiB");
    StereoArgs a;
    stereo_args(e, e, 0, 1, d_images, d_images + frame_step, row_step, 2 * frame_step, kp_capacity, bf, min_z, a);
    a.kps = d_kps;
    a.desc = d_desc;
    a.counts = d_counts;
    a.uright = d_uright;
    a.depth = d_depth;
    const size_t nsad = (size_t)npairs * kp_capacity;
    const hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
    {
        std::lock_guard<std::mutex> lk(e->stereo_mu);
        orbgpu_extractor::SadScratch* sc = nullptr;
        for (auto& x : e->stereo_sad)
            if (x.stream == hs) sc = &x;
        if (!sc) {
            e->stereo_sad.push_back({hs, {}, 0});
            sc = &e->stereo_sad.back();
        }
        if (nsad > sc->n) {
            sc->n = 0;
            ORB_HIP(hipMalloc((void**)sc->d.put(), nsad * sizeof(int)));  // (put() frees the smaller one)
            sc->n = nsad;
        }
        a.sad = sc->d;
    }
    ORB_HIP(launch_stereo(a, npairs, hs));
    return ORBGPU_OK;
}

// ComputeStereoMatches of a stereo Frame built by two extractors
// (Frame.cpp:84-98): the pyramids of their last orbgpu_extract calls, read in
// place in HBM; keypoints / descriptors from the host.
int orbgpu_stereo_matches_pair(orbgpu_extractor* left, orbgpu_extractor* right, const orbgpu_keypoint* kps_l,
                               const uint8_t* desc_l, int n_l, const orbgpu_keypoint* kps_r, const uint8_t* desc_r,
                               int n_r, float bf, float min_z, float* uright, float* depth) {
    if (!left || !right || n_l < 0 || n_r < 0 || (n_l > 0 && (!kps_l || !desc_l || !uright || !depth)) ||
        (n_r > 0 && (!kps_r || !desc_r)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    DeviceScope ds_(left->device);
    if (left->p.width != right->p.width || left->p.height != right->p.height ||
        left->p.nlevels != right->p.nlevels || left->p.scale_factor != right->p.scale_factor)
        return fail(ORBGPU_ERR_ARG, "left and right extractors differ in geometry");
    if (!left->last_img || !right->last_img || left->last_batch < 1 || right->last_batch < 1)
        return fail(ORBGPU_ERR_ARG, "both extractors need an extraction first");
    if (left->last_row != right->last_row) return fail(ORBGPU_ERR_ARG, "level-0 row steps differ");
    // frame capacity a multiple of 64, so the staged L and R arrays are contiguous (28 * 64 and
    // 32 * 64 bytes are multiples of the arena's 256-byte granule): frame f at + f * cap
    const int cap = (std::max(std::max(n_l, n_r), 1) + 63) / 64 * 64;
    if (cap > 65535) return fail(ORBGPU_ERR_ARG, "more than 65535 keypoints");
    if (stereo_lds_bytes(cap, left->geo.g.lv[0].h) > 160 * 1024)
        return fail(ORBGPU_ERR_UNSUPPORTED, "stereo LDS tables exceed 160 KiB");
    if (n_l == 0) return ORBGPU_OK;
    int rc = check_device();
    if (rc) return rc;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    // the pyramids were written on the extractors' streams (orbgpu_extract returned after
    // synchronising them), so the thread's stream may read them directly
    HostCall call(*ctx);
    orbgpu_keypoint *dk, *dk_r;
    uint8_t *dd, *dd_r;
    int* dn;
    float *du, *dz;
    int* ds;
    const int counts[2] = {n_l, n_r};
    rc = call.run([&](HostCall& A) {
        dk = A.inout(kps_l, (size_t)n_l, (size_t)cap);
        dk_r = A.inout(kps_r, (size_t)n_r, (size_t)cap);
        dd = A.inout(desc_l, 32 * (size_t)n_l, 32 * (size_t)cap);
        dd_r = A.inout(desc_r, 32 * (size_t)n_r, 32 * (size_t)cap);
        dn = A.in(counts, 2);
        du = A.out<float>((size_t)cap);
        dz = A.out<float>((size_t)cap);
        ds = A.out<int>((size_t)cap);
    });
    if (rc) return rc;
    if (dk_r != dk + cap || dd_r != dd + 32 * (size_t)cap) return fail(ORBGPU_ERR_ARG, "internal: staging layout");
    StereoArgs a;
    stereo_args(left, right, 0, 0, left->last_img, right->last_img, left->last_row, 0, cap, bf, min_z, a);
    a.kps = dk;
    a.desc = dd;
    a.counts = dn;
    a.uright = du;
    a.depth = dz;
    a.sad = ds;
    ORB_HIP(launch_stereo(a, 1, ctx->stream));
    call.fetch(du, uright, 4 * (size_t)n_l);
    call.fetch(dz, depth, 4 * (size_t)n_l);
    return call.finish();
}

}  // extern "C"
