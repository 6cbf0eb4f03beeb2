// geometry.cpp -- the per-extractor geometry (geometry.h), computed once with
// the reference's own float arithmetic: ORBextractor.cpp:412-472, :781-795,
// :545-547, :1127-1128 and OpenCV-2.4 resize()'s tap tables.  Host arithmetic
// only: no HIP runtime call.
#include "geometry.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "host_common.h"

namespace orbgpu {

namespace {

// OpenCV 2.4 cvRound / cvFloor on the host (SSE2 cvtsd2si = half to even)
inline int cv_round(double v) { return (int)std::nearbyint(v); }
inline int cv_floor(double v) { const int i = cv_round(v); return i - (v < (double)i); }
inline int sat_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

int vresize_simd_end(int width) {
    int x = 0;
    while (x <= width - 16) x += 16;
    while (x < width - 4) x += 4;
    return x;
}

// resize(src sw x sh -> dw x dh, INTER_LINEAR) tap tables, as cv::resize
// (2.4, imgwarp.cpp) computes xofs/ialpha and yofs/ibeta for 8U.
void build_resize_tables(int sw, int sh, int dw, int dh, std::vector<int2>& xt, std::vector<int2>& yt) {
    const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
    const double scale_x = 1.0 / inv_sx, scale_y = 1.0 / inv_sy;
    xt.resize(dw);
    yt.resize(dh);
    int xmax = dw;
    std::vector<int> sxs(dw), a0s(dw), a1s(dw);
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; }
        }
        sxs[dx] = sx;
        a0s[dx] = sat_s16(cv_round((1.f - fx) * 2048.f));
        a1s[dx] = sat_s16(cv_round(fx * 2048.f));
    }
    for (int dx = 0; dx < dw; ++dx) {
        int sx0 = sxs[dx], sx1 = sxs[dx] + 1, a0 = a0s[dx], a1 = a1s[dx];
        if (dx >= xmax) { sx1 = sx0; a0 = 2048; a1 = 0; }  // HResizeLinear tail: S[sx]*ONE
        xt[dx].x = sx0 | (sx1 << 16);
        xt[dx].y = (a0 & 0xFFFF) | (a1 << 16);
    }
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= (float)sy;
        const int b0 = sat_s16(cv_round((1.f - fy) * 2048.f)), b1 = sat_s16(cv_round(fy * 2048.f));
        const int y0 = std::min(std::max(sy, 0), sh - 1), y1 = std::min(std::max(sy + 1, 0), sh - 1);
        yt[dy].x = y0 | (y1 << 16);
        yt[dy].y = (b0 & 0xFFFF) | (b1 << 16);
    }
}

// row pitch of pyramid levels >= 1 in HBM (bytes)
#ifndef ORBGPU_PYR_PITCH_ALIGN
#define ORBGPU_PYR_PITCH_ALIGN 16
#endif

}  // namespace

int build_geometry(const ExtractorParams& p, ExtractorGeometry& o, GeometryTables& t) {
    std::vector<int4>& ptab = t.ptab;
    std::vector<int2>& ytab = t.ytab;
    std::vector<int2>* xtab = t.with_xtab ? &t.xtab : nullptr;
    const int L = p.nlevels;
    o.scale.assign(L, 1.f);
    o.sigma2.assign(L, 1.f);
    for (int i = 1; i < L; ++i) {
        o.scale[i] = o.scale[i - 1] * p.scale_factor;
        o.sigma2[i] = o.scale[i] * o.scale[i];
    }
    o.inv_scale.resize(L);
    o.inv_sigma2.resize(L);
    for (int i = 0; i < L; ++i) {
        o.inv_scale[i] = 1.0f / o.scale[i];
        o.inv_sigma2[i] = 1.0f / o.sigma2[i];
    }
    std::vector<int> nfeat(L);
    const float factor = 1.0f / p.scale_factor;
    float per_scale = p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; ++l) {
        nfeat[l] = cv_round(per_scale);
        sum += nfeat[l];
        per_scale *= factor;
    }
    nfeat[L - 1] = std::max(p.nfeatures - sum, 0);

    Geom& g = o.g;
    std::memset(&g, 0, sizeof(g));
    g.nlevels = L;
    g.width = p.width;
    g.height = p.height;
    g.ini_th = std::min(std::max(p.ini_th, 0), 255);
    g.min_th = std::min(std::max(p.min_th, 0), 255);
    size_t pyr_off = 0, cand_off = 0;
    int cell_base = 0, out_off = 0, max_cells = 0, ncap = 0;
    ptab.clear();
    ytab.clear();
    if (xtab) xtab->clear();
    for (int l = 0; l < L; ++l) {
        LevelGeom& v = g.lv[l];
        v.w = cv_round((float)p.width * o.inv_scale[l]);
        v.h = cv_round((float)p.height * o.inv_scale[l]);
        v.scale = o.scale[l];
        v.size_i = (int)(31 * o.scale[l]);
        v.nfeat = nfeat[l];
        v.pitch = (int)round_up((size_t)v.w, l == 0 ? 16 : ORBGPU_PYR_PITCH_ALIGN);
        if (l > 0) {
            v.frame_bytes = (size_t)v.pitch * v.h;
            v.offset = pyr_off;
            pyr_off += round_up(v.frame_bytes * p.max_batch, 256);
        }
        // cells
        v.max_bx = v.w - kEdge + 3;
        v.max_by = v.h - kEdge + 3;
        const float width = (float)(v.max_bx - kBorder), height = (float)(v.max_by - kBorder);
        if (!(width >= 30.f && height >= 30.f))
            return fail(ORBGPU_ERR_UNSUPPORTED, "level " + std::to_string(l) + " is smaller than one FAST cell");
        v.ncols = (int)(width / 30.f);
        v.nrows = (int)(height / 30.f);
        v.wcell = (int)std::ceil(width / v.ncols);
        v.hcell = (int)std::ceil(height / v.nrows);
        if (v.wcell + 9 > kMaxWin || v.hcell + 6 > kMaxWin)
            return fail(ORBGPU_ERR_UNSUPPORTED, "FAST cell window larger than the LDS tile");
        if (v.max_bx - kBorder > 2047 || v.max_by - kBorder > 2047)
            return fail(ORBGPU_ERR_UNSUPPORTED, "levels wider/taller than 2079 px are not supported");
        v.cell_base = cell_base;
        v.cell_cap = ((v.wcell + 1) / 2) * ((v.hcell + 1) / 2);
        v.cand_offset = cand_off;
        cell_base += v.ncols * v.nrows;
        cand_off += (size_t)v.ncols * v.nrows * v.cell_cap;
        max_cells = std::max(max_cells, v.ncols * v.nrows);
        // octree roots (:545-547)
        v.nini = (int)std::round((float)(v.max_bx - kBorder) / (float)(v.max_by - kBorder));
        if (v.nini < 1) return fail(ORBGPU_ERR_UNSUPPORTED, "image aspect gives zero initial octree nodes");
        v.hx = (float)(v.max_bx - kBorder) / v.nini;
        v.ocap = std::max(v.nfeat + 3, 4 * v.nini);
        v.out_offset = out_off;
        out_off += v.ocap;
        ncap = std::max(ncap, std::max(v.ocap, v.nini));
        // resize tables: ytab rows as built; columns as per-quad tap records
        // for pyramid.hip (3 int4 per quad: (lo, wt) x 4 and the 4 perm selectors)
        if (l > 0) {
            const LevelGeom& pl = g.lv[l - 1];
            std::vector<int2> xt, yt;
            build_resize_tables(pl.w, pl.h, v.w, v.h, xt, yt);
            for (const int2& t : xt)  // Q11 weights: non-negative, a0 + a1 = 2048 (+-1)
                if ((t.y & 0xFFFF) > 2049 || (t.y >> 16) < 0 || (t.y & 0xFFFF) + (t.y >> 16) > 2049)
                    return fail(ORBGPU_ERR_UNSUPPORTED, "unexpected resize weights");
            v.simd_end = vresize_simd_end(v.w);
            const int quads = (v.w + 3) / 4;
            if (quads < 3) return fail(ORBGPU_ERR_UNSUPPORTED, "pyramid level narrower than 9 px");
            // pyramid.hip gives the last quad (the scalar tail) its own lanes
            // (or, when w is a multiple of 16, there is no tail at all)
            if (v.simd_end == v.w && v.w % 4 == 0) v.qmain = quads;
            else if (v.simd_end == 4 * (quads - 1)) v.qmain = quads - 1;
            else return fail(ORBGPU_ERR_UNSUPPORTED, "resize tail is not the last quad");
            if ((size_t)v.pitch * v.h >= (1u << 31)) return fail(ORBGPU_ERR_UNSUPPORTED, "level too large");
            v.ptab_offset = (int)ptab.size();
            // Column taps per quad for pyramid.hip (3 int4 per quad):
            //   (w0, wt0, wt1, wt2), (wt3, sel0, sel1, sel2), (sel3, 0, 0, 0).
            // The kernel reads the three dwords d0, d1, d2 at byte w0 of the
            // source row; pixels 0..2 take their two taps from (d1:d0) and
            // pixel 3 from (d2:d1) with v_perm_b32 (selector sel_k puts the
            // tap bytes in the HIGH byte of each 16-bit lane, i.e. x256), and
            // wt_k = (16 ialpha0, 16 ialpha1) so v_dot2_u32_u16 yields
            // 4096 x the exact HResizeLinear sum: its high half is h >> 4,
            // the operand of VResizeLinearVec_32s8u.  w0 may be -4 or -8
            // (the LDS ring rows have 16 bytes in front).  Holds for every
            // scale factor <= 2 (checked here per quad).
            for (int q = 0; q < quads; ++q) {
                const int lo = xt[4 * q].x & 0xFFFF;
                int w0 = 0, sel[4] = {0, 0, 0, 0};
                bool ok = false;
                for (int c = 0; c < 3 && !ok; ++c) {
                    w0 = (lo & ~3) - 4 * c;
                    ok = true;
                    for (int k = 0; k < 4; ++k) {
                        const int dx = 4 * q + k;
                        if (dx >= v.w) { sel[k] = (int)0x0c0c0c0cu; continue; }
                        const int base = w0 + (k == 3 ? 4 : 0);
                        const int t0 = (xt[dx].x & 0xFFFF) - base;
                        const int t1 = ((xt[dx].y >> 16) != 0 ? (xt[dx].x >> 16) : (xt[dx].x & 0xFFFF)) - base;
                        if (t0 < 0 || t1 > 7 || t1 < t0) { ok = false; break; }
                        sel[k] = (int)(0x000c000cu | ((uint32_t)t0 << 8) | ((uint32_t)t1 << 24));
                    }
                }
                if (!ok) return fail(ORBGPU_ERR_UNSUPPORTED, "pyramid column taps do not fit a 12-byte window (scale factor > 2?)");
                if (q > 0 && w0 < 0) return fail(ORBGPU_ERR_UNSUPPORTED, "pyramid column window before the row start");
                int wt[4];
                for (int k = 0; k < 4; ++k) {
                    const int dx = 4 * q + k;
                    const uint32_t a0 = dx < v.w ? (uint32_t)(xt[dx].y & 0xFFFF) : 0u;
                    const uint32_t a1 = dx < v.w ? (uint32_t)(xt[dx].y >> 16) : 0u;
                    wt[k] = (int)((a0 << 4) | (a1 << 20));
                }
                ptab.push_back(int4{w0, wt[0], wt[1], wt[2]});
                ptab.push_back(int4{wt[3], sel[0], sel[1], sel[2]});
                ptab.push_back(int4{sel[3], 0, 0, 0});
            }
            v.ytab_offset = (int)ytab.size();
            ytab.insert(ytab.end(), yt.begin(), yt.end());
            if (xtab) {
                v.xtab_offset = (int)xtab->size();
                xtab->insert(xtab->end(), xt.begin(), xt.end());
            }
        }
    }
    {
        const int rc = plan_pyramid(g, ytab, ptab, p.max_batch, o.pyr_plan);
        if (rc) return rc;
    }
    g.total_cells = cell_base;
    g.cand_frame = cand_off;
    g.slots_frame = out_off;
    g.cells_magic = udiv40_magic((uint32_t)cell_base);
    g.slots_magic = udiv40_magic((uint32_t)out_off);
    for (int l = 0; l < kMaxLevels; ++l) {
        g.lvl_cell_base[l] = l < L ? g.lv[l].cell_base : INT_MAX;
        g.lvl_out_offset[l] = l < L ? g.lv[l].out_offset : INT_MAX;
    }
    g.max_cells_level = max_cells;
    size_t blur_off = 0;
    int tiles = 0;
    for (int l = 0; l < L; ++l) {
        LevelGeom& v = g.lv[l];
        v.blur_frame_bytes = (size_t)v.pitch * v.h;
        v.blur_offset = blur_off;
        blur_off += round_up(v.blur_frame_bytes * p.max_batch, 256);
        v.blur_tiles_x = (v.w + 3) / 4;
        v.blur_tile_base = tiles;
        tiles += v.blur_tiles_x * ((v.h + kBlurStrip - 1) / kBlurStrip);
    }
    g.blur_tiles_frame = tiles;
    o.blur_bytes = blur_off + 256;  // slack: describe reads 40-byte row spans
    g.win_pitch = 0;
    g.win_rows = 0;
    g.det_max = 0;
    for (int l = 0; l < L; ++l) {
        if (g.lv[l].wcell > 61) return fail(ORBGPU_ERR_UNSUPPORTED, "FAST cell wider than 61 px");
        // window = cell + 6 px, starting at tile column 1 or 5 (fast.hip's column shift)
        g.win_pitch = std::max(g.win_pitch, (int)round_up((size_t)g.lv[l].wcell + 11, 4));
        g.win_rows = std::max(g.win_rows, g.lv[l].hcell + 6);
        g.det_max = std::max(g.det_max, (int)round_up((size_t)g.lv[l].wcell * g.lv[l].hcell, 8));
    }
    // fast.hip is instantiated for window pitches 40, 48, ..., 72 (compile-time
    // ring offsets)
    g.win_pitch = g.win_pitch <= 40 ? 40 : (int)round_up((size_t)g.win_pitch, 8);
    o.pyr_bytes = pyr_off;
    o.max_kps = out_off;
    o.ncap = (int)round_up((size_t)ncap, 16);
    if (o.ncap > 4096) return fail(ORBGPU_ERR_UNSUPPORTED, "more than 4092 features per level");
    // octree.hip's main pass scans (children << 16 | survives) in one int:
    // C <= 4 * nodes must stay below 2^15 and S <= nodes below 2^16
    static_assert(4 * 4096 < (1 << 15), "octree packed scan bound");
    if (4 * o.ncap >= (1 << 15)) return fail(ORBGPU_ERR_UNSUPPORTED, "octree node capacity exceeds the packed scan");
    // Key capacity (a multiple of 64) for a requested one: the keys and their node
    // indices (6 bytes a key) in the requested LDS bytes less 64, and the whole
    // workgroup within 64 KiB; a level with more candidates uses HBM scratch.
    // keys in LDS (4 B key + 2 B node id each) for a request of `req` keys, in
    // steps of 64, shrunk until the workgroup's LDS fits 64 KiB: a request of
    // 2560 yields 2560 (round 5 subtracted a leftover 64 B and got 2496)
    auto key_capacity = [&g](int req, int ncap_) {
        const long bytes = (long)round_up((size_t)req * 4, 16) + (long)round_up((size_t)req * 2, 16);
        int kc = bytes > 0 ? (int)(bytes / 6) & ~63 : 0;
        while (kc > 0 && octree_lds_bytes(g, kc, ncap_) > 65536) kc -= 64;
        return kc;
    };
    // Two level groups in one octree launch: levels 0..1 (below), the
    // smaller levels with node arrays for their own feature counts and keys in LDS up to
    // ~2048; a level with more candidates takes the same HBM-scratch path as an oversized
    // big level.  The launch's LDS per workgroup is the larger group's.
    const int split = std::min(2, L);
    int ncap_b = 0;
    for (int l = split; l < L; ++l) ncap_b = std::max(ncap_b, std::max(g.lv[l].ocap, g.lv[l].nini));
    ncap_b = (int)round_up((size_t)std::max(ncap_b, 1), 16);
    // levels 0..1: keys in LDS up to ~2560 (26.1 KiB at 640x480: six workgroups per CU;
    // with 4096, four -- round 5: octree 0.158 -> 0.136 ms per 512 frames,
    // profiles/r05_notes_ab.txt r6c, r7a).  The bench stream's levels 0-1 have
    // ~1,000-1,300 candidates; a level with more than the capacity takes the HBM-scratch
    // path (correct, slower), as an oversized level always did.  ORBGPU_OCT_KCAP_A
    // overrides the 2560 (256..4096).
    // read at every create: test_gpu_parity.py::test_octree_key_scratch_path_matches_oracle switches it in-process
    const int kcap_a_env = env_now_int("ORBGPU_OCT_KCAP_A", 2560);
    const int kcap_a_req = kcap_a_env >= 256 && kcap_a_env <= 4096 ? kcap_a_env : 2560;
    o.oct_groups[0] = OctreeGroup{0, split, key_capacity(kcap_a_req, o.ncap), o.ncap};
    o.oct_groups[1] = OctreeGroup{split, L - split, key_capacity(2048, ncap_b), ncap_b};
    return ORBGPU_OK;
}

std::vector<uint32_t> build_index_tables(const Geom& g) {
    std::vector<uint32_t> tab((size_t)g.total_cells + g.slots_frame);
    for (int l = 0; l < g.nlevels; ++l) {
        const LevelGeom& v = g.lv[l];
        for (int c = 0; c < v.ncols * v.nrows; ++c)
            tab[(size_t)v.cell_base + c] = (uint32_t)l | (uint32_t)(c / v.ncols) << 4 | (uint32_t)(c % v.ncols) << 18;
        for (int i = 0; i < v.ocap; ++i) tab[(size_t)g.total_cells + v.out_offset + i] = (uint32_t)l | (uint32_t)i << 4;
    }
    return tab;
}

}  // namespace orbgpu
