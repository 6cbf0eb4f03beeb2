// geometry.h -- the extractor geometry as a value: everything that depends
// only on the ORBextractor parameters and the frame size, computed on the host
// (geometry.cpp) without a device.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "orbgpu_internal.h"
#include "orbgpu_kernels.h"

namespace orbgpu {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct ExtractorParams {
    int nfeatures = 0;
    float scale_factor = 0.f;
    int nlevels = 0, ini_th = 0, min_th = 0;
    int width = 0, height = 0, max_batch = 0;
};

struct ExtractorGeometry {
    Geom g;  // (cell_tab / slot_tab: device pointers, set by the extractor after the upload)
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    PyrPlan pyr_plan;                // fused pyramid pass: row records, tick ranges, per-lane entries
    OctreeGroup oct_groups[2] = {};  // the octree launches (big levels / small levels)
    int ncap = 0, max_kps = 0;
    size_t pyr_bytes = 0, blur_bytes = 0;
};

// resize tap tables of levels 1..L-1: per-quad column records (pyramid.hip),
// row taps, and -- when with_xtab -- the per-column taps of the level-by-level pyramid
struct GeometryTables {
    std::vector<int4> ptab;
    std::vector<int2> ytab, xtab;
    bool with_xtab = false;
};

// ORBextractor ctor arithmetic (ORBextractor.cpp:417-448) + per-level layout;
// ORBGPU_ERR_UNSUPPORTED (message in orbgpu_last_error) for a geometry the kernels do not take
int build_geometry(const ExtractorParams& p, ExtractorGeometry& o, GeometryTables& t);

// per-cell / per-slot lookup tables (Geom::cell_tab, then slot_tab)
std::vector<uint32_t> build_index_tables(const Geom& g);

}  // namespace orbgpu
