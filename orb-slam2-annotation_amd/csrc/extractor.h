// extractor.h -- the orbgpu_extractor handle (private to extractor.cpp,
// extractor_debug.cpp and stereo.cpp): the geometry, the HBM buffers sized for
// max_batch frames, the single-frame staging, streams and events.  Built only
// by orbgpu_extractor_create; every buffer is owned by its holder.
#pragma once

#include <array>
#include <mutex>
#include <optional>
#include <vector>

#include "../../include/orbgpu.h"
#include "geometry.h"
#include "host_common.h"

struct orbgpu_extractor {
    // first member, so destroyed last: the destructor releases every handle
    // below under the extractor's device, then the thread's device comes back
    std::optional<orbgpu::DeviceScope> dtor_scope;
    int device = -1;  // the HIP device the handle's buffers and stream live on
    orbgpu::ExtractorParams p;
    orbgpu::ExtractorGeometry geo;
    // device buffers
    orbgpu::DevBuf<uint8_t> d_pyr;
    orbgpu::DevBuf<uint8_t> d_blur;  // blurred levels (debug API), on first use
    orbgpu::DevBuf<int4> d_ptab;
    orbgpu::DevBuf<int4> d_pyr_ent;
    orbgpu::DevBuf<int2> d_pyr_tab;
    orbgpu::DevBuf<int2> d_xtab;  // level-by-level pyramid (small batches): column / row taps per level
    orbgpu::DevBuf<int2> d_ytab;
    orbgpu::DevBuf<int4> d_band;  // banded pyramid (small batches): per band and level row ranges
    orbgpu::DevBuf<uint32_t> d_cand;
    orbgpu::DevBuf<int> d_cell_counts;
    orbgpu::DevBuf<uint32_t> d_gkeys;
    orbgpu::DevBuf<uint16_t> d_gknode;
    orbgpu::DevBuf<uint32_t> d_oct_out;
    orbgpu::DevBuf<uint32_t> d_tab;  // cell_tab then slot_tab (Geom)
    orbgpu::DevBuf<int> d_oct_count;
    orbgpu::DevBuf<int> d_err;
    orbgpu::DevBuf<int> d_trace;  // optional octree pass trace (debug API)
    // ComputeStereoMatches: accepted SAD per left keypoint (pairs x cap), one scratch per
    // stream the batch form was called on (calls on different streams never share one)
    struct SadScratch {
        hipStream_t stream;
        orbgpu::DevBuf<int> d;
        size_t n;
    };
    std::vector<SadScratch> stereo_sad;
    std::mutex stereo_mu;
    // host-image path
    orbgpu::DevBuf<uint8_t> d_img;
    orbgpu::DevBuf<uint8_t> fg_img;  // host-mapped fine-grained HBM staging of the single-frame upload (knob)
    size_t img_pitch = 0;
    // one device block [count, err, pad, pad | keypoints(cap) | descriptors(cap)]
    // mirrored by one pinned host block, so a frame's outputs come back in a
    // single asynchronous copy
    orbgpu::DevBuf<uint8_t> d_single;
    orbgpu::PinBuf<uint8_t> h_single;
    orbgpu::PinBuf<uint8_t> h_img;  // staging of the host image (img_pitch rows)
    orbgpu::PinBuf<unsigned long long> h_done;  // coherent: the single-frame completion flag (done_flag_kernel)
    unsigned long long done_seq = 0;            // the last issued call's flag value (0: none pending)
    orbgpu::PinBuf<uint8_t> h_levels;  // staging of one frame's pyramid (copy_levels), on first use
    size_t single_bytes = 0, single_desc_off = 0;
    orbgpu_keypoint* d_kps1 = nullptr;  // (into d_single)
    uint8_t* d_desc1 = nullptr;
    int* d_count1 = nullptr;
    orbgpu::Stream stream;
    // octree / describe chunk pipeline (run_batch): describe of chunk c on aux_stream
    // while the octree of chunk c+1 runs on the batch stream; on first use
    orbgpu::Stream aux_stream;
    std::array<orbgpu::Event, 9> od_ev;  // [c]: octree of chunk c done; [8]: the describes done
    // stage timing
    bool profile = false;
    hipEvent_t stage_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // the caller's (orbgpu_extractor_set_stage_event)
    std::vector<std::array<orbgpu::Event, 5>> ev;
    size_t ev_used = 0;
    // last extraction (for copy_level)
    const uint8_t* last_img = nullptr;
    size_t last_row = 0, last_frame = 0;
    int last_batch = 0;

    ~orbgpu_extractor() { dtor_scope.emplace(device); }
};
