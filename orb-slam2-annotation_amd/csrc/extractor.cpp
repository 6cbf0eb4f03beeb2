// extractor.cpp -- the extractor's C ABI (include/orbgpu.h): create / destroy /
// info, the launch sequence of one extraction
//   pyramid level 1..L-1  ->  FAST cells (all levels)  ->  octree (frame x
//   level)  ->  angle + blur + rBRIEF + keypoint fields (one wave per slot),
// the single-frame host path and the pyramid read-back.
// Errors raised inside kernels (capacity overflows) are accumulated in a
// device word and reported by orbgpu_extractor_sync(); nothing is silently
// truncated.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>

#include "extractor.h"

using namespace orbgpu;

namespace {

// batches up to this size take the level-by-level pyramid (ORBGPU_PYR_LEVELS_MAX_BATCH overrides)
int pyr_levels_max_batch() { return ORB_ENV_ONCE_INT("ORBGPU_PYR_LEVELS_MAX_BATCH", 8); }

// chunks of the octree / describe pipeline (ORBGPU_OD_CHUNKS, 1..8; 1 = the plain
// sequence): the octree of chunk c+1 (latency bound) runs beside the describe of
// chunk c (VALU bound)
int od_chunks() {
    // read per batch: test_gpu_parity.py::test_batch_octree_describe_chunks_match_oracle switches it in-process
    const int n = env_now_int("ORBGPU_OD_CHUNKS", 1);
    return n < 1 ? 1 : (n > 8 ? 8 : n);
}

// the single-frame path moves the frame in and the results out by kernels over
// PCIe (a copy kernel reading pinned memory; describe writing the results into
// pinned memory) -- ORBGPU_SINGLE_ZEROCOPY=0 selects copy-engine transfers
bool single_zero_copy() { return ORB_ENV_ONCE_FLAG("ORBGPU_SINGLE_ZEROCOPY", true); }

// the single-frame call waits on a completion flag written by a one-wave kernel
// after the extraction (ORBGPU_SINGLE_DONE_FLAG=0: hipStreamSynchronize)
bool single_done_flag() { return ORB_ENV_ONCE_FLAG("ORBGPU_SINGLE_DONE_FLAG", true); }

// The single-frame upload: the host writes the frame straight into host-mapped
// fine-grained HBM (write-combined over PCIe, ~7.5 us for 640x480) and the
// extraction reads it there -- no copy kernel (a memcpy into pinned memory,
// 2 us, then a copy kernel reading it over PCIe, 9.5 us).  Drop-in
// ORBextractor::operator() 87-91 -> 78-81 us with the completion flag
// (profiles/r06_notes_ab.txt r6p).  ORBGPU_SINGLE_VRAM_STAGING=0, or an
// allocation the device refuses: the pinned staging and the copy kernel.
bool single_vram_staging() { return ORB_ENV_ONCE_FLAG("ORBGPU_SINGLE_VRAM_STAGING", true); }

// ORBGPU_OCT_FUSED=0 selects the octree's pass-by-pass main loop (A/B and parity
// checks); read per batch: tests/test_octree_fused.py switches it in-process
bool oct_fused() { return env_now_int("ORBGPU_OCT_FUSED", 1) != 0; }

// ORBGPU_PYR_BANDS=0 selects the level-by-level launches (A/B and parity checks)
bool pyr_bands_off() { return !ORB_ENV_ONCE_FLAG("ORBGPU_PYR_BANDS", true); }

int run_batch(orbgpu_extractor* e, const uint8_t* imgs, int batch, size_t row_step, size_t frame_step,
              orbgpu_keypoint* kps, uint8_t* desc, int* counts, int kp_cap, hipStream_t s, int* err_copy = nullptr) {
    const Geom& g = e->geo.g;
    Event* evs = nullptr;
    if (e->profile) {
        if (e->ev_used == e->ev.size()) {
            std::array<Event, 5> a;
            // (timing only: no system-scope fence on record, which stalled the
            // stream before its next kernel)
            for (Event& x : a) ORB_HIP(hipEventCreateWithFlags(x.put(), hipEventDisableSystemFence));
            e->ev.push_back(std::move(a));
        }
        evs = e->ev[e->ev_used++].data();
        ORB_HIP(hipEventRecord(evs[0], s));
    }
    // the tick pipeline is one block per frame: a few frames go in row bands
    // over the chip (one launch), or level by level when no band plan fits
    if (batch <= pyr_levels_max_batch() && g.bd_nb > 0 && !pyr_bands_off())
        ORB_HIP(launch_pyramid_bands(g, batch, e->d_band, e->d_xtab, e->d_ytab, imgs, row_step, frame_step, e->d_pyr, s));
    else if (batch <= pyr_levels_max_batch())
        ORB_HIP(launch_pyramid_levels(g, batch, e->d_xtab, e->d_ytab, imgs, row_step, frame_step, e->d_pyr, s));
    else
        ORB_HIP(launch_pyramid(g, batch, e->d_pyr_ent, e->d_pyr_tab, imgs, row_step, frame_step, e->d_pyr, s));
    if (evs) ORB_HIP(hipEventRecord(evs[1], s));
    if (e->stage_ev[0]) ORB_HIP(hipEventRecord(e->stage_ev[0], s));
    ORB_HIP(launch_fast_cells(g, batch, imgs, row_step, frame_step, e->d_pyr, e->d_cand, e->d_cell_counts, e->d_err, s));
    if (evs) ORB_HIP(hipEventRecord(evs[2], s));
    if (e->stage_ev[1]) ORB_HIP(hipEventRecord(e->stage_ev[1], s));
    const int nch = (err_copy || batch < 16 * od_chunks()) ? 1 : od_chunks();
    if (nch == 1) {
        ORB_HIP(launch_octree(g, batch, e->d_cand, e->d_cell_counts, e->d_gkeys, e->d_gknode, e->d_oct_out,
                              e->d_oct_count, e->d_err, e->geo.oct_groups, 2, e->d_trace, oct_fused(), s));
        if (evs) ORB_HIP(hipEventRecord(evs[3], s));
        if (e->stage_ev[2]) ORB_HIP(hipEventRecord(e->stage_ev[2], s));
        // GaussianBlur is fused into describe (blur of each keypoint's patch);
        // whole blurred levels exist only for the debug API (round 5: blurring
        // the upper levels whole and sampling them was slower)
        ORB_HIP(launch_describe(g, batch, imgs, row_step, frame_step, e->d_pyr, e->d_oct_out, e->d_oct_count, kps,
                                desc, counts, kp_cap, s, err_copy ? e->d_err.get() : nullptr, err_copy));
    } else {
        // the octree chunks in order on s, each chunk's describe on the aux stream after
        // its octree: describe(c) overlaps octree(c+1); s joins the aux stream at the end
        if (!e->aux_stream) {
            int lo = 0, hi = 0;
            ORB_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
            ORB_HIP(hipStreamCreateWithPriority(e->aux_stream.put(), hipStreamNonBlocking, hi));
            for (Event& x : e->od_ev) ORB_HIP(hipEventCreateWithFlags(x.put(), hipEventDisableTiming));
        }
        hipStream_t a = e->aux_stream;
        for (int c = 0; c < nch; ++c) {
            const int f0 = batch * c / nch, f1 = batch * (c + 1) / nch, nb = f1 - f0;
            ORB_HIP(launch_octree(g, nb, e->d_cand + (size_t)f0 * g.cand_frame,
                                  e->d_cell_counts + (size_t)f0 * g.total_cells,
                                  e->d_gkeys + (size_t)f0 * g.cand_frame, e->d_gknode + (size_t)f0 * g.cand_frame,
                                  e->d_oct_out + (size_t)f0 * g.slots_frame, e->d_oct_count + (size_t)f0 * kOcStride,
                                  e->d_err, e->geo.oct_groups, 2, c == 0 ? e->d_trace.get() : nullptr, oct_fused(), s));
            // the octree stage ends with the last chunk's octree (the describes of the
            // earlier chunks overlap it on the aux stream; describe = the rest)
            if (c == nch - 1 && evs) ORB_HIP(hipEventRecord(evs[3], s));
            ORB_HIP(hipEventRecord(e->od_ev[c], s));
            ORB_HIP(hipStreamWaitEvent(a, e->od_ev[c], 0));
            ORB_HIP(launch_describe(g, nb, imgs, row_step, frame_step, e->d_pyr, e->d_oct_out, e->d_oct_count, kps,
                                    desc, counts, kp_cap, a, nullptr, nullptr, f0));
        }
        if (e->stage_ev[2]) ORB_HIP(hipEventRecord(e->stage_ev[2], s));
        ORB_HIP(hipEventRecord(e->od_ev[8], a));
        ORB_HIP(hipStreamWaitEvent(s, e->od_ev[8], 0));
    }
    if (evs) ORB_HIP(hipEventRecord(evs[4], s));
    if (e->stage_ev[3]) ORB_HIP(hipEventRecord(e->stage_ev[3], s));
    e->last_img = imgs;
    e->last_row = row_step;
    e->last_frame = frame_step;
    e->last_batch = batch;
    return ORBGPU_OK;
}

std::string capacity_message(int err) {
    std::string m = "kernel capacity overflow:";
    if (err & kErrCellCap) m += " FAST-cell";
    if (err & kErrNodeCap) m += " octree-nodes";
    if (err & kErrKeyCap) m += " octree-keys";
    if (err & kErrSeqCap) m += " octree-seq";
    return m;
}

int collect_errors(orbgpu_extractor* e, hipStream_t s) {
    ORB_HIP(hipStreamSynchronize(s));
    int err = 0;
    ORB_HIP(hipMemcpy(&err, e->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (err) {
        ORB_HIP(hipMemset(e->d_err, 0, sizeof(int)));
        return fail(ORBGPU_ERR_CAPACITY, capacity_message(err));
    }
    return ORBGPU_OK;
}

template <class T>
hipError_t upload(T* dst, const std::vector<T>& src) {
    return src.empty() ? hipSuccess : hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace

extern "C" {

int orbgpu_extractor_create(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th, int width,
                            int height, int max_batch, orbgpu_extractor** out) {
    if (!out) return fail(ORBGPU_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (nfeatures <= 0 || nlevels <= 0 || nlevels > kMaxLevels || !(scale_factor > 1.f) || width <= 0 ||
        height <= 0 || max_batch <= 0)
        return fail(ORBGPU_ERR_ARG, "invalid extractor parameters");
    int rc = check_device();
    if (rc) return rc;
    // (every failure below frees what was built: the handle owns its buffers)
    auto e = std::make_unique<orbgpu_extractor>();
    ORB_HIP(hipGetDevice(&e->device));
    e->p = ExtractorParams{nfeatures, scale_factor, nlevels, ini_th, min_th, width, height, max_batch};
    GeometryTables t;
    t.with_xtab = true;
    rc = build_geometry(e->p, e->geo, t);
    if (rc) return rc;
    std::vector<int4> bands;
    plan_pyramid_bands(e->geo.g, t.ytab, bands);
    const Geom& g = e->geo.g;
    const PyrPlan& plan = e->geo.pyr_plan;
    const size_t B = (size_t)max_batch;
    e->img_pitch = round_up((size_t)width, 16);
    if ((rc = dalloc(e->d_pyr, e->geo.pyr_bytes)) || (rc = dalloc(e->d_ptab, t.ptab.size())) ||
        (rc = dalloc(e->d_cand, g.cand_frame * B)) ||
        (rc = dalloc(e->d_cell_counts, (size_t)g.total_cells * B)) || (rc = dalloc(e->d_gkeys, g.cand_frame * B)) ||
        (rc = dalloc(e->d_gknode, g.cand_frame * B)) || (rc = dalloc(e->d_oct_out, (size_t)g.slots_frame * B)) ||
        (rc = dalloc(e->d_oct_count, (size_t)kOcStride * B)) || (rc = dalloc(e->d_err, 1)) ||
        (rc = dalloc(e->d_img, e->img_pitch * height)) ||
        (rc = dalloc(e->d_pyr_ent, plan.ent.size())) || (rc = dalloc(e->d_pyr_tab, plan.tab.size())) ||
        (rc = dalloc(e->d_xtab, t.xtab.size())) || (rc = dalloc(e->d_ytab, t.ytab.size())) ||
        (rc = dalloc(e->d_band, std::max<size_t>(bands.size(), 1))) ||
        (rc = dalloc(e->d_tab, (size_t)g.total_cells + g.slots_frame)))
        return rc;
    if (upload(e->d_tab.get(), build_index_tables(g)) != hipSuccess) return fail(ORBGPU_ERR_HIP, "table upload failed");
    e->geo.g.cell_tab = e->d_tab;
    e->geo.g.slot_tab = e->d_tab + g.total_cells;
    e->single_desc_off = round_up(16 + (size_t)e->geo.max_kps * sizeof(orbgpu_keypoint), 256);
    e->single_bytes = e->single_desc_off + (size_t)e->geo.max_kps * 32;
    if ((rc = dalloc(e->d_single, e->single_bytes))) return rc;
    e->d_count1 = reinterpret_cast<int*>(e->d_single.get());
    e->d_kps1 = reinterpret_cast<orbgpu_keypoint*>(e->d_single + 16);
    e->d_desc1 = e->d_single + e->single_desc_off;
    // (the output block coherent with the flag: describe's stores go straight
    // to host memory, so the flag written after them orders them for the host)
    if (hipHostMalloc((void**)e->h_single.put(), e->single_bytes,
                      single_done_flag() ? hipHostMallocCoherent : hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)e->h_img.put(), e->img_pitch * height, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)e->h_done.put(), 64, hipHostMallocCoherent) != hipSuccess)
        return fail(ORBGPU_ERR_HIP, "pinned staging allocation failed");
    __atomic_store_n(e->h_done.get(), 0ull, __ATOMIC_RELEASE);
    if (single_vram_staging() &&
        hipExtMallocWithFlags((void**)e->fg_img.put(), e->img_pitch * height, hipDeviceMallocFinegrained) != hipSuccess)
        (void)e->fg_img.release();  // (the pinned staging and the copy kernel then)
    if (hipMemcpy(e->d_ptab, t.ptab.data(), t.ptab.size() * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess ||
        upload(e->d_xtab.get(), t.xtab) != hipSuccess || upload(e->d_ytab.get(), t.ytab) != hipSuccess ||
        upload(e->d_band.get(), bands) != hipSuccess || upload(e->d_pyr_ent.get(), plan.ent) != hipSuccess ||
        upload(e->d_pyr_tab.get(), plan.tab) != hipSuccess ||
        pyramid_set_lds_limit(g) != hipSuccess ||
        hipMemset(e->d_err, 0, sizeof(int)) != hipSuccess ||
        hipStreamCreateWithFlags(e->stream.put(), hipStreamNonBlocking) != hipSuccess)
        return fail(ORBGPU_ERR_HIP, "buffer initialisation failed");
    *out = e.release();
    return ORBGPU_OK;
}

int orbgpu_extractor_create_on_device(int device, int nfeatures, float scale_factor, int nlevels, int ini_th,
                                      int min_th, int width, int height, int max_batch, orbgpu_extractor** out) {
    if (out) *out = nullptr;
    int rc = validate_device(device);
    if (rc) return rc;
    DeviceScope ds(device);
    return orbgpu_extractor_create(nfeatures, scale_factor, nlevels, ini_th, min_th, width, height, max_batch, out);
}

int orbgpu_extractor_destroy(orbgpu_extractor* handle) {
    delete handle;
    return ORBGPU_OK;
}

int orbgpu_extractor_get_info_sized(const orbgpu_extractor* e, orbgpu_extractor_info* info, size_t info_size) {
    if (!e || !info) return fail(ORBGPU_ERR_ARG, "NULL argument");
    if (info_size == 0) return fail(ORBGPU_ERR_ARG, "info_size is 0");
    orbgpu_extractor_info full;
    const int rc = orbgpu_extractor_get_info(e, &full);
    if (rc) return rc;
    std::memcpy(info, &full, std::min(info_size, sizeof(full)));
    return ORBGPU_OK;
}

int orbgpu_extractor_get_info(const orbgpu_extractor* e, orbgpu_extractor_info* info) {
    if (!e || !info) return fail(ORBGPU_ERR_ARG, "NULL argument");
    std::memset(info, 0, sizeof(*info));
    info->nlevels = e->p.nlevels;
    info->width = e->p.width;
    info->height = e->p.height;
    info->max_batch = e->p.max_batch;
    info->max_keypoints = e->geo.max_kps;
    info->device = e->device;
    for (int l = 0; l < e->p.nlevels && l < 32; ++l) {
        info->level_width[l] = e->geo.g.lv[l].w;
        info->level_height[l] = e->geo.g.lv[l].h;
        info->features_per_level[l] = e->geo.g.lv[l].nfeat;
        info->level_capacity[l] = e->geo.g.lv[l].ocap;
    }
    return ORBGPU_OK;
}

int orbgpu_extractor_get_scales(const orbgpu_extractor* e, float* s, float* is, float* s2, float* is2) {
    if (!e) return fail(ORBGPU_ERR_ARG, "NULL extractor");
    for (int l = 0; l < e->p.nlevels; ++l) {
        if (s) s[l] = e->geo.scale[l];
        if (is) is[l] = e->geo.inv_scale[l];
        if (s2) s2[l] = e->geo.sigma2[l];
        if (is2) is2[l] = e->geo.inv_sigma2[l];
    }
    return ORBGPU_OK;
}

int orbgpu_extract_batch_device(orbgpu_extractor* e, const uint8_t* imgs, int batch, size_t row_step,
                                size_t frame_step, orbgpu_keypoint* kps, uint8_t* desc, int* counts,
                                int kp_cap, void* stream) {
    if (!e || !imgs || !kps || !desc || !counts) return fail(ORBGPU_ERR_ARG, "NULL argument");
    DeviceScope ds_(e->device);
    if (batch <= 0 || batch > e->p.max_batch) return fail(ORBGPU_ERR_ARG, "batch outside [1, max_batch]");
    if (kp_cap < e->geo.max_kps) return fail(ORBGPU_ERR_CAPACITY, "kp_capacity < max_keypoints");
    if (row_step < (size_t)e->p.width || row_step % 16 || ((uintptr_t)imgs & 15) || (batch > 1 && frame_step % 16) ||
        (batch > 1 && frame_step < row_step * e->p.height))
        return fail(ORBGPU_ERR_ARG, "images must be 16-byte aligned with row_step and frame_step multiples of 16");
    return run_batch(e, imgs, batch, row_step, frame_step, kps, desc, counts, kp_cap, (hipStream_t)stream);
}

int orbgpu_extractor_sync(orbgpu_extractor* e, void* stream) {
    if (!e) return fail(ORBGPU_ERR_ARG, "NULL extractor");
    DeviceScope ds_(e->device);
    return collect_errors(e, (hipStream_t)stream);
}

// orbgpu_extract in two halves: issue (host image -> staging -> HBM,
// extraction, results towards the pinned output block; nothing waited for)
// and finish (one stream synchronisation, then the results out of the pinned
// block).  orbgpu_extract_pair issues two extractors' frames from one thread
// before finishing either.
static int extract_issue(orbgpu_extractor* e, const uint8_t* image, int width, int height, size_t step) {
    if (width != e->p.width || height != e->p.height)
        return fail(ORBGPU_ERR_ARG, "image size differs from the extractor geometry");
    if (step < (size_t)width) return fail(ORBGPU_ERR_ARG, "step < width");
    hipStream_t s = e->stream;
    const int max_kps = e->geo.max_kps;
    if (single_zero_copy()) {
        // the drop-in (Frame constructor) path without copy-engine transfers:
        // host image -> pinned staging (one memcpy for a continuous image) ->
        // a copy kernel into HBM; extraction with describe writing keypoints,
        // descriptors, the count and the error word straight into the pinned
        // output block
        uint8_t* stage = e->fg_img ? e->fg_img.get() : e->h_img.get();
        if (step == e->img_pitch)
            std::memcpy(stage, image, step * (size_t)height);
        else
            for (int y = 0; y < height; ++y)
                std::memcpy(stage + (size_t)y * e->img_pitch, image + (size_t)y * step, width);
        if (!e->fg_img) ORB_HIP(launch_copy16(e->d_img, e->h_img, e->img_pitch * (size_t)height, s));
        const int rc = run_batch(e, e->fg_img ? e->fg_img.get() : e->d_img.get(), 1, e->img_pitch, e->img_pitch * height,
                                 reinterpret_cast<orbgpu_keypoint*>(e->h_single + 16), e->h_single + e->single_desc_off,
                                 reinterpret_cast<int*>(e->h_single.get()), max_kps, s,
                                 reinterpret_cast<int*>(e->h_single + 4));
        if (rc || !single_done_flag()) return rc;
        static std::atomic<unsigned long long> next_seq{1};  // distinct across extractors and calls
        const unsigned long long seq = next_seq.fetch_add(1, std::memory_order_relaxed);
        ORB_HIP(launch_done_flag(e->h_done, seq, s));
        e->done_seq = seq;
        return ORBGPU_OK;
    }
    // the drop-in path with copy-engine transfers: host image -> pinned
    // staging -> one async H2D; extraction; the error word folded into the
    // output block; one async D2H of the whole block (in four row bands: the
    // DMA of band i overlaps the host copy of band i+1)
    constexpr int kBands = 4;
    for (int b = 0; b < kBands; ++b) {
        const int y0 = height * b / kBands, y1 = height * (b + 1) / kBands;
        if (y1 <= y0) continue;
        if (step == e->img_pitch)  // a continuous cv::Mat of a 16-multiple width: one copy per band
            std::memcpy(e->h_img + (size_t)y0 * step, image + (size_t)y0 * step, step * (size_t)(y1 - y0));
        else
            for (int y = y0; y < y1; ++y)
                std::memcpy(e->h_img + (size_t)y * e->img_pitch, image + (size_t)y * step, width);
        ORB_HIP(hipMemcpyAsync(e->d_img + (size_t)y0 * e->img_pitch, e->h_img + (size_t)y0 * e->img_pitch,
                               e->img_pitch * (size_t)(y1 - y0), hipMemcpyHostToDevice, s));
    }
    // describe moves the error word into the output block and clears it
    int rc = run_batch(e, e->d_img, 1, e->img_pitch, e->img_pitch * height, e->d_kps1, e->d_desc1, e->d_count1,
                       max_kps, s, reinterpret_cast<int*>(e->d_single + 4));
    if (rc) return rc;
    ORB_HIP(hipMemcpyAsync(e->h_single, e->d_single, e->single_bytes, hipMemcpyDeviceToHost, s));
    return ORBGPU_OK;
}

// the call's completion: its flag (spun on; after 20 ms, or with no flag
// pending, the stream is synchronised, which also reports a failed kernel)
static int wait_single(orbgpu_extractor* e) {
    const unsigned long long seq = e->done_seq;
    e->done_seq = 0;
    if (seq) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 1;; ++it) {
            if (__atomic_load_n(e->h_done.get(), __ATOMIC_ACQUIRE) == seq) return ORBGPU_OK;
            if ((it & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
            __builtin_ia32_pause();
        }
    }
    ORB_HIP(hipStreamSynchronize(e->stream));
    return ORBGPU_OK;
}

static int extract_finish(orbgpu_extractor* e, orbgpu_keypoint* keypoints, uint8_t* descriptors, int capacity,
                          int* n) {
    if (int rc = wait_single(e)) return rc;
    int count = 0, err = 0;
    std::memcpy(&count, e->h_single, sizeof(int));
    std::memcpy(&err, e->h_single + 4, sizeof(int));
    if (err) return fail(ORBGPU_ERR_CAPACITY, capacity_message(err));
    if (count > capacity) return fail(ORBGPU_ERR_CAPACITY, "keypoint capacity too small");
    if (count > 0) {
        if (keypoints) std::memcpy(keypoints, e->h_single + 16, (size_t)count * sizeof(orbgpu_keypoint));
        if (descriptors) std::memcpy(descriptors, e->h_single + e->single_desc_off, (size_t)count * 32);
    }
    *n = count;
    return ORBGPU_OK;
}

int orbgpu_extract(orbgpu_extractor* e, const uint8_t* image, int width, int height, size_t step,
                   orbgpu_keypoint* keypoints, uint8_t* descriptors, int capacity, int* n) {
    if (!e || !n) return fail(ORBGPU_ERR_ARG, "NULL argument");
    DeviceScope ds_(e->device);
    if (!image || width <= 0 || height <= 0) {  // ORBextractor.cpp:1056
        *n = -1;
        return ORBGPU_OK;
    }
    int rc = extract_issue(e, image, width, height, step);
    if (rc) return rc;
    return extract_finish(e, keypoints, descriptors, capacity, n);
}

int orbgpu_extract_pair(orbgpu_extractor* e0, const uint8_t* image0, size_t step0, orbgpu_keypoint* keypoints0,
                        uint8_t* descriptors0, int capacity0, int* n0, orbgpu_extractor* e1, const uint8_t* image1,
                        size_t step1, orbgpu_keypoint* keypoints1, uint8_t* descriptors1, int capacity1, int* n1,
                        int width, int height) {
    if (!e0 || !e1 || !n0 || !n1) return fail(ORBGPU_ERR_ARG, "NULL argument");
    if (e0 == e1) return fail(ORBGPU_ERR_ARG, "the two frames need two extractors");
    const bool empty = !image0 || !image1 || width <= 0 || height <= 0;
    if (empty) {  // ORBextractor.cpp:1056, per image
        *n0 = *n1 = -1;
        int rc = ORBGPU_OK;
        if (image0 && width > 0 && height > 0)
            rc = orbgpu_extract(e0, image0, width, height, step0, keypoints0, descriptors0, capacity0, n0);
        if (!rc && image1 && width > 0 && height > 0)
            rc = orbgpu_extract(e1, image1, width, height, step1, keypoints1, descriptors1, capacity1, n1);
        return rc;
    }
    int rc;
    {
        DeviceScope ds_(e0->device);
        rc = extract_issue(e0, image0, width, height, step0);
    }
    if (rc) {
        DeviceScope ds_(e0->device);
        (void)hipStreamSynchronize(e0->stream);  // nothing of frame 0 is left in flight
        return rc;
    }
    int rc1;
    {
        DeviceScope ds_(e1->device);
        rc1 = extract_issue(e1, image1, width, height, step1);
    }
    {
        DeviceScope ds_(e0->device);
        rc = extract_finish(e0, keypoints0, descriptors0, capacity0, n0);
    }
    DeviceScope ds_(e1->device);
    if (rc1) {
        (void)hipStreamSynchronize(e1->stream);
        return rc1;
    }
    const int r1 = extract_finish(e1, keypoints1, descriptors1, capacity1, n1);
    return rc ? rc : r1;
}

int orbgpu_extractor_profile(orbgpu_extractor* e, int enable) {
    if (!e) return fail(ORBGPU_ERR_ARG, "NULL extractor");
    e->profile = enable != 0;
    return ORBGPU_OK;
}

int orbgpu_extractor_set_stage_event(orbgpu_extractor* e, int stage, void* event) {
    if (!e || stage < 0 || stage > 3) return fail(ORBGPU_ERR_ARG, "invalid argument");
    e->stage_ev[stage] = (hipEvent_t)event;
    return ORBGPU_OK;
}

int orbgpu_extractor_stage_times(orbgpu_extractor* e, float* ms4, int* nbatches, int reset) {
    if (!e) return fail(ORBGPU_ERR_ARG, "NULL extractor");
    DeviceScope ds_(e->device);
    float acc[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < e->ev_used; ++i) {
        ORB_HIP(hipEventSynchronize(e->ev[i][4]));
        for (int k = 0; k < 4; ++k) {
            float ms = 0.f;
            ORB_HIP(hipEventElapsedTime(&ms, e->ev[i][k], e->ev[i][k + 1]));
            acc[k] += ms;
        }
    }
    if (ms4)
        for (int k = 0; k < 4; ++k) ms4[k] = acc[k];
    if (nbatches) *nbatches = (int)e->ev_used;
    if (reset) e->ev_used = 0;
    return ORBGPU_OK;
}

int orbgpu_extractor_copy_level(orbgpu_extractor* e, int frame, int level, uint8_t* dst, size_t dst_step) {
    if (!e || !dst) return fail(ORBGPU_ERR_ARG, "NULL argument");
    DeviceScope ds_(e->device);
    if (!e->last_img || frame < 0 || frame >= e->last_batch || level < 0 || level >= e->p.nlevels)
        return fail(ORBGPU_ERR_ARG, "no such frame/level in the last extraction");
    const LevelGeom& v = e->geo.g.lv[level];
    if (dst_step < (size_t)v.w) return fail(ORBGPU_ERR_ARG, "dst_step < level width");
    const uint8_t* src = level == 0 ? e->last_img + (size_t)frame * e->last_frame
                                    : e->d_pyr + v.offset + (size_t)frame * v.frame_bytes;
    const size_t pitch = level == 0 ? e->last_row : (size_t)v.pitch;
    ORB_HIP(hipStreamSynchronize(e->stream));
    ORB_HIP(hipMemcpy2D(dst, dst_step, src, pitch, v.w, v.h, hipMemcpyDeviceToHost));
    return ORBGPU_OK;
}

// mvImagePyramid of one frame: every level into pinned staging with one async
// copy each on the extractor's stream, one synchronisation, then host copies
// into the caller's rows (a pageable 2-D copy per level costs ~1 ms)
int orbgpu_extractor_copy_levels(orbgpu_extractor* e, int frame, uint8_t* const* dst, const size_t* dst_step) {
    if (!e || !dst || !dst_step) return fail(ORBGPU_ERR_ARG, "NULL argument");
    DeviceScope ds_(e->device);
    if (!e->last_img || frame < 0 || frame >= e->last_batch)
        return fail(ORBGPU_ERR_ARG, "no such frame in the last extraction");
    const Geom& g = e->geo.g;
    size_t total = 0, off[kMaxLevels];
    for (int l = 0; l < g.nlevels; ++l) {
        const LevelGeom& v = g.lv[l];
        if (!dst[l] || dst_step[l] < (size_t)v.w) return fail(ORBGPU_ERR_ARG, "bad destination of a level");
        off[l] = total;
        total += round_up((size_t)v.pitch * v.h, 256);
    }
    if (!e->h_levels) ORB_HIP(hipHostMalloc((void**)e->h_levels.put(), total, hipHostMallocDefault));
    // level 0 of the last single-frame call is still in the pinned upload
    // staging (pinned-staging path); other levels, and level 0 otherwise (the
    // fine-grained HBM staging, a batch), come back by one copy kernel writing
    // the pinned staging (no copy-engine transfers; a level 0 whose rows do not
    // fit the staging's level-0 pitch by a 2-D copy)
    const bool l0_host = single_zero_copy() && e->last_img == e->d_img && e->last_batch == 1;
    const uint8_t* l0_dev = e->last_img + (size_t)frame * e->last_frame;
    const bool l0_kernel = !l0_host && e->last_row <= (size_t)g.lv[0].pitch &&
                           (((uintptr_t)l0_dev | e->last_row * g.lv[0].h) & 15) == 0;
    if (!l0_host && !l0_kernel)
        ORB_HIP(hipMemcpy2DAsync(e->h_levels, (size_t)g.lv[0].pitch, l0_dev, e->last_row, g.lv[0].w,
                                 g.lv[0].h, hipMemcpyDeviceToHost, e->stream));
    if (g.nlevels > 1 || l0_kernel) {
        CopyList16 L{};
        L.n = 0;
        if (l0_kernel) L.d[L.n++] = CopyDesc16{l0_dev, e->h_levels + off[0], e->last_row * g.lv[0].h};
        for (int l = 1; l < g.nlevels && L.n < kCopyList; ++l) {
            const LevelGeom& v = g.lv[l];
            L.d[L.n++] = CopyDesc16{e->d_pyr + v.offset + (size_t)frame * v.frame_bytes, e->h_levels + off[l],
                                    (size_t)v.pitch * v.h};
        }
        ORB_HIP(launch_copy16_list(L, e->stream));
    }
    ORB_HIP(hipStreamSynchronize(e->stream));
    for (int l = 0; l < g.nlevels; ++l) {
        const LevelGeom& v = g.lv[l];
        const uint8_t* src = l == 0 && l0_host ? e->h_img.get() : e->h_levels + off[l];
        const size_t sp = l == 0 && (l0_host || l0_kernel) ? (l0_host ? e->img_pitch : e->last_row) : (size_t)v.pitch;
        for (int y = 0; y < v.h; ++y) std::memcpy(dst[l] + (size_t)y * dst_step[l], src + (size_t)y * sp, (size_t)v.w);
    }
    return ORBGPU_OK;
}

}  // extern "C"
