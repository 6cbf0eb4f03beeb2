// extractor_debug.cpp -- the stage-level debug ABI (include/orbgpu_debug.h):
// accessors of the last extraction, and the CPU-only runs of the fused pyramid
// plan, which need the geometry but no extractor and no device.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/orbgpu_debug.h"
#include "extractor.h"

using namespace orbgpu;

namespace {

// the geometry of the CPU-only entry points (one frame; the thresholds do not matter to the pyramid)
int plan_geometry(int nfeatures, float scale_factor, int nlevels, int width, int height, ExtractorGeometry& geo,
                  GeometryTables& t) {
    return build_geometry(ExtractorParams{nfeatures, scale_factor, nlevels, 20, 7, width, height, 1}, geo, t);
}

}  // namespace

extern "C" {

int orbgpu_debug_level_blur(orbgpu_extractor* e, int frame, int level, uint8_t* dst, size_t dst_step) {
    if (!e || !dst) return fail(ORBGPU_ERR_ARG, "NULL argument");
    DeviceScope ds_(e->device);
    if (!e->last_img || frame < 0 || frame >= e->last_batch || level < 0 || level >= e->p.nlevels)
        return fail(ORBGPU_ERR_ARG, "no such frame/level in the last extraction");
    const LevelGeom& v = e->geo.g.lv[level];
    if (dst_step < (size_t)v.w) return fail(ORBGPU_ERR_ARG, "dst_step < level width");
    ORB_HIP(hipStreamSynchronize(e->stream));
    // the product path never materialises blurred levels: blur the last
    // batch's levels on demand (same arithmetic as describe's fused blur)
    if (!e->d_blur) {
        int rc = dalloc(e->d_blur, e->geo.blur_bytes);
        if (rc) return rc;
    }
    ORB_HIP(launch_blur_levels(e->geo.g, e->last_batch, e->last_img, e->last_row, e->last_frame, e->d_pyr, e->d_blur,
                               e->stream));
    ORB_HIP(hipStreamSynchronize(e->stream));
    ORB_HIP(hipMemcpy2D(dst, dst_step, e->d_blur + v.blur_offset + (size_t)frame * v.blur_frame_bytes, v.pitch, v.w,
                        v.h, hipMemcpyDeviceToHost));
    return ORBGPU_OK;
}

int orbgpu_debug_level_candidates(orbgpu_extractor* e, int frame, int level, int* xys, int cap) {
    if (!e || frame < 0 || frame >= e->last_batch || level < 0 || level >= e->p.nlevels)
        return fail(ORBGPU_ERR_ARG, "no such frame/level in the last extraction");
    DeviceScope ds_(e->device);
    const Geom& g = e->geo.g;
    const LevelGeom& v = g.lv[level];
    const int ncells = v.ncols * v.nrows;
    std::vector<int> counts(ncells);
    std::vector<uint32_t> slots((size_t)ncells * v.cell_cap);
    ORB_HIP(hipStreamSynchronize(e->stream));
    ORB_HIP(hipDeviceSynchronize());
    ORB_HIP(hipMemcpy(counts.data(), e->d_cell_counts + (size_t)frame * g.total_cells + v.cell_base,
                      ncells * sizeof(int), hipMemcpyDeviceToHost));
    ORB_HIP(hipMemcpy(slots.data(), e->d_cand + (size_t)frame * g.cand_frame + v.cand_offset,
                      slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    int n = 0;
    for (int c = 0; c < ncells; ++c)
        for (int k = 0; k < counts[c]; ++k, ++n)
            if (n < cap && xys) {
                const uint32_t key = slots[(size_t)c * v.cell_cap + k];
                xys[3 * n] = key_x(key); xys[3 * n + 1] = key_y(key); xys[3 * n + 2] = key_s(key);
            }
    return n;
}

int orbgpu_debug_octree_trace(orbgpu_extractor* e, int enable, int* out, int cap) {
    if (!e) return fail(ORBGPU_ERR_ARG, "NULL extractor");
    DeviceScope ds_(e->device);
    const size_t n = (size_t)kMaxLevels * 512;
    if (enable && !e->d_trace) {
        ORB_HIP(hipMalloc((void**)e->d_trace.put(), n * sizeof(int)));
        ORB_HIP(hipMemset(e->d_trace, 0, n * sizeof(int)));
    }
    if (out && e->d_trace) {
        ORB_HIP(hipDeviceSynchronize());
        ORB_HIP(hipMemcpy(out, e->d_trace, std::min(n, (size_t)cap) * sizeof(int), hipMemcpyDeviceToHost));
    }
    return ORBGPU_OK;
}

int orbgpu_debug_level_octree(orbgpu_extractor* e, int frame, int level, int* xys, int cap) {
    if (!e || frame < 0 || frame >= e->last_batch || level < 0 || level >= e->p.nlevels)
        return fail(ORBGPU_ERR_ARG, "no such frame/level in the last extraction");
    DeviceScope ds_(e->device);
    const Geom& g = e->geo.g;
    const LevelGeom& v = g.lv[level];
    int n = 0;
    ORB_HIP(hipDeviceSynchronize());
    ORB_HIP(hipMemcpy(&n, e->d_oct_count + (size_t)frame * kOcStride + level, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<uint32_t> keys(std::max(n, 1));
    ORB_HIP(hipMemcpy(keys.data(), e->d_oct_out + (size_t)frame * g.slots_frame + v.out_offset,
                      (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < n && i < cap && xys; ++i) {
        xys[3 * i] = key_x(keys[i]); xys[3 * i + 1] = key_y(keys[i]); xys[3 * i + 2] = key_s(keys[i]);
    }
    return n;
}

int orbgpu_debug_pyramid_emulate(int nfeatures, float scale_factor, int nlevels, int width, int height,
                                 const uint8_t* img, size_t img_step, uint8_t* out, size_t out_bytes, int* info) {
    if (!img || !out || nfeatures <= 0 || nlevels <= 0 || nlevels > kMaxLevels || !(scale_factor > 1.f) ||
        width <= 0 || height <= 0 || img_step < (size_t)width)
        return fail(ORBGPU_ERR_ARG, "invalid emulation arguments");
    ExtractorGeometry geo;  // host geometry only: no device is touched
    GeometryTables t;
    int rc = plan_geometry(nfeatures, scale_factor, nlevels, width, height, geo, t);
    if (rc) return rc;
    const Geom& g = geo.g;
    size_t need = 0;
    for (int l = 1; l < nlevels; ++l) need += (size_t)g.lv[l].w * g.lv[l].h;
    if (out_bytes < need) return fail(ORBGPU_ERR_CAPACITY, "out_bytes smaller than levels 1..L-1");
    std::vector<std::vector<uint8_t>> levels;
    rc = emulate_pyramid(g, t.ytab, geo.pyr_plan, img, img_step, levels);
    if (rc) return rc;
    for (int l = 1; l < nlevels; ++l) {
        std::memcpy(out, levels[(size_t)l].data(), levels[(size_t)l].size());
        out += levels[(size_t)l].size();
    }
    if (info) {
        const int v[8] = {g.tk_ticks, g.tk_t0, g.tk_cwaves, g.tk_pwaves, g.tk_np, g.tk_e, g.tk_lds_bytes,
                          g.lv[0].tk_ring_rows};
        std::memcpy(info, v, sizeof(v));
    }
    return ORBGPU_OK;
}

// The octree launch's plan for these parameters (no GPU): per level group its
// first level, level count, keys and nodes held in LDS, and LDS bytes.
int orbgpu_debug_octree_plan(int nfeatures, float scale_factor, int nlevels, int width, int height, int* out) {
    if (!out || nfeatures <= 0 || nlevels <= 0 || nlevels > kMaxLevels || !(scale_factor > 1.f) || width <= 0 ||
        height <= 0)
        return fail(ORBGPU_ERR_ARG, "invalid octree plan arguments");
    ExtractorGeometry geo;  // host geometry only: no device is touched
    GeometryTables t;
    const int rc = plan_geometry(nfeatures, scale_factor, nlevels, width, height, geo, t);
    if (rc) return rc;
    for (int i = 0; i < 2; ++i) {
        const OctreeGroup& G = geo.oct_groups[i];
        const int v[5] = {G.level0, G.nlev, G.kcap, G.ncap, (int)octree_lds_bytes(geo.g, G.kcap, G.ncap)};
        std::memcpy(out + 5 * i, v, sizeof(v));
    }
    return ORBGPU_OK;
}

// The fused pyramid plan's work per tick (tools/pyr_plan_cost.py): rows[k *
// lanes + i] = the rows lane i (entry 0, then entry 1 at i + CL) computes at
// tick k; lane_info[i] = level | tail << 8 (level 0: an idle lane); dims =
// {ticks, lanes, compute waves, entries per lane}.
int orbgpu_debug_pyramid_plan_rows(int nfeatures, float scale_factor, int nlevels, int width, int height,
                                   int* rows, size_t rows_n, int* lane_info, size_t lanes_n, int* dims) {
    if (!dims || nfeatures <= 0 || nlevels < 2 || nlevels > kMaxLevels || !(scale_factor > 1.f) || width <= 0 ||
        height <= 0)
        return fail(ORBGPU_ERR_ARG, "invalid plan arguments");
    ExtractorGeometry geo;
    GeometryTables t;
    int rc = plan_geometry(nfeatures, scale_factor, nlevels, width, height, geo, t);
    if (rc) return rc;
    const Geom& g = geo.g;
    const int K = g.tk_ticks, CL = 64 * g.tk_cwaves, E = g.tk_e, n = CL * E;
    dims[0] = K;
    dims[1] = n;
    dims[2] = g.tk_cwaves;
    dims[3] = E;
    if (!rows || !lane_info) return ORBGPU_OK;
    if (rows_n < (size_t)K * n || lanes_n < (size_t)n) return fail(ORBGPU_ERR_CAPACITY, "plan output too small");
    const uint32_t* rng = reinterpret_cast<const uint32_t*>(geo.pyr_plan.tab.data()) + g.tk_rng;
    for (int i = 0; i < n; ++i) {
        const int4* r = &geo.pyr_plan.ent[(size_t)i * 9];
        lane_info[i] = r[2].w | (r[0].y ? 1 << 8 : 0);
        for (int k = 0; k < K; ++k) rows[(size_t)k * n + i] = (int)((rng[(size_t)k * g.tk_rs + r[0].x] >> 11) & 31u);
    }
    return ORBGPU_OK;
}

}  // extern "C"
