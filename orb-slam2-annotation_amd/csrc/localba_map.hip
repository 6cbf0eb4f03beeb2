// localba_map.hip -- the two host stretches of Optimizer::LocalBundleAdjustment on the device
// (include/orbgpu_localba_map.h), against the map mirror of orbgpu_localmap.h and batched over
// independent keyframes: the gather that writes localba.hip's input arrays, and the collection of
// vToErase with the write-back into the mirror.  localba.hip runs unchanged between the two.
//
//  orbgpu_local_ba_gather_batch_device (src/Optimizer.cpp:540-752), ten launches:
//    1 lg_clear_kernel    (chunk, job)    the job's marks and keys in the workspace
//    2 lg_locals_kernel   (job)           pKF and its covisibles: first occurrences by an atomic min of
//                                         the list index, the non-bad ones compacted in list order
//                                         (:544-555); the exclusive sum of the list's slot counts, which
//                                         numbers every (list position, slot) pair
//    3 lg_mark_kernel     (keyframe, job) atomic min of that number over each good point's slots: its
//                                         first occurrence (:560-576)
//    4 lg_count_kernel    (keyframe, job) the first occurrences per keyframe
//    5 lg_points_kernel   (keyframe, job) first occurrences compacted in slot order: the point list
//    6 lg_sight_kernel    (point, job)    a wave per local point over its observations: every id checked;
//                                         a keyframe that is not marked local gets the atomic min of
//                                         (point position, observation position), its first sight
//                                         (:590-592); the point's edges (:688) and the job's monocular
//                                         ones are counted
//    7 lg_fixed_kernel    (point, job)    per point the observations that own a non-bad fixed keyframe
//    8 lg_finish_kernel   (job)           the exclusive sums of both counts over the points; the status,
//                                         the result, the prepared orbgpu_localba_job, local_kfs and the
//                                         local poses
//    9 lg_place_kernel    (point, job)    the fixed cameras at their positions (fixed_kfs, their poses),
//                                         the points (local_points, Xw)
//   10 lg_edges_kernel    (point, job)    each of the eight edge arrays written once
//  orbgpu_local_ba_collect_batch_device (:813-884), two launches:
//    1 lc_erase_kernel    (job)           the flagged monocular edges compacted in edge order, then the
//                                         flagged stereo edges
//    2 lc_write_kernel    (chunk, job)    Tcw_out rows 0-2 and Xw_out to the mirror's kf_Tcw and pos
//
// Marks and counts are integer atomics, exact in any order; positions come from prefix sums in key
// order and floats are copied, never computed, so every output byte is a function of the job and
// the mirrors.  No launch waits for another workgroup; nothing synchronises with the host.  Every
// id read from the job or the mirrors is range-checked before it is used as an index; a job with
// one out of range ends as BAD_JOB, and all output arrays are written by launches 8-10, after the
// last check.
#include "../../include/orbgpu_localba_map.h"
#include "host_common.h"
#include "ransac_device.h"

namespace orbgpu {

namespace {

using namespace ransacdev;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGridY = 1024;  // the (keyframe, job) and (point, job) launches stride over the rest
constexpr unsigned kNoKey = 0xffffffffu;
constexpr unsigned long long kNoSight = ~0ull;
constexpr int kUnmarked = -1, kUnlisted = -2;  // kfmark: not local; marked local but bad (:552-554)

enum { kPending = -1 };

struct GState {  // a job between the launches
    int status;  // kPending until lg_finish_kernel, ORBGPU_LOCALBA_MAP_BAD_JOB from lg_locals_kernel
    int bad;     // written by launches 3 and 6 only: an id out of range
    int skip;    // the slots exceed ORBGPU_LOCALBA_MAP_MAX_SLOTS: no point is looked for
    int n_local;
    int n_points;  // summed by lg_count_kernel
    int n_mono;    // summed by lg_sight_kernel
    int n_fixed;
    int n_edges;
};

struct GWork {  // the opaque block, carved
    GState* st;
    unsigned long long* fkey;  // per job and keyframe: its first sight from a local point, or kNoSight
    unsigned* kfkey;           // per job and keyframe: 0 for pKF, 1 + its first index in covis_all, or kNoKey
    int* kfmark;               // per job and keyframe: the local position, kUnmarked or kUnlisted
    int* fpos;                 // per job and fixed keyframe: its pose index
    int* list;                 // per job: the local keyframes, all of them
    int* kfbase;               // per job and list position: the slots before it
    int* cnt;                  // per job and list position: first occurrences
    unsigned* key;             // per job and point: the number of its first (list position, slot), or kNoKey
    int* ptlist;               // per job: the local points, all of them
    int* ecnt;                 // per job and local point: its edges, then (ebase) the edges before it
    int* fcnt;                 // per job and local point: the fixed cameras it is the first to see
    int* ebase;
    int* fbase;
};

inline GWork carve(void* base, int n, int n_kf, int n_pt, size_t* bytes) {
    const size_t N = (size_t)(n > 0 ? n : 1), NK = (size_t)(n_kf > 0 ? n_kf : 1), NP = (size_t)(n_pt > 0 ? n_pt : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    GWork v;
    v.st = take<GState>(p, N);
    v.fkey = take<unsigned long long>(p, N * NK);
    v.kfkey = take<unsigned>(p, N * NK);
    v.kfmark = take<int>(p, N * NK);
    v.fpos = take<int>(p, N * NK);
    v.list = take<int>(p, N * NK);
    v.kfbase = take<int>(p, N * NK);
    v.cnt = take<int>(p, N * NK);
    v.key = take<unsigned>(p, N * NP);
    v.ptlist = take<int>(p, N * NP);
    v.ecnt = take<int>(p, N * NP);
    v.fcnt = take<int>(p, N * NP);
    v.ebase = take<int>(p, N * NP);
    v.fbase = take<int>(p, N * NP);
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return v;
}

struct Dims {
    int kf_stride, pose_stride, point_stride, edge_stride;
};

struct Out {  // the gather's output arrays
    orbgpu_localba_gather_result* results;
    orbgpu_localba_job* ba_jobs;
    float* Tcw;
    uint8_t* fixed;
    float* cam;
    float* Xw;
    int* edge_pose;
    int* edge_point;
    float* obs;
    float* inv_sigma2;
    int* local_kfs;
    int* fixed_kfs;
    int* local_points;
    int* edge_kf;
    int* edge_slot;
};

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

// offset + count within an array of `total`
__device__ __forceinline__ bool span_ok(int off, int cnt, int total) {
    return off >= 0 && cnt >= 0 && (long long)off + cnt <= (long long)total;
}

// the sum of v over the block; every thread calls it, s_red holds kWaves values
__device__ __forceinline__ long long block_sum(long long v, long long* s_red) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();  // s_red may still be read from the call before
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int w = 0; w < kWaves; ++w) t += s_red[w];
    return t;
}

// The exclusive prefix of c over the block's stripe plus `before`, which then moves past the stripe.
// Every thread calls it; s_red holds kWaves values.
__device__ __forceinline__ long long stripe_prefix(long long c, long long& before, long long* s_red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = c;
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    __syncthreads();
    if (lane == 63) s_red[wave] = incl;
    __syncthreads();
    long long pre = before, tot = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) pre += s_red[w];
        tot += s_red[w];
    }
    before += tot;
    return pre + incl - c;
}

__device__ __forceinline__ size_t kf_base(int k, int n_kf) { return (size_t)k * (n_kf > 0 ? n_kf : 1); }
__device__ __forceinline__ size_t pt_base(int k, int n_pt) { return (size_t)k * (n_pt > 0 ? n_pt : 1); }

// pose row p of job k from keyframe kf
__device__ __forceinline__ void copy_pose(const Out& O, const orbgpu_map_mirror_ba& B, size_t row, int kf, uint8_t fixed) {
    for (int c = 0; c < 12; ++c) O.Tcw[12 * row + c] = B.kf_Tcw[12 * (size_t)kf + c];
    for (int c = 0; c < 5; ++c) O.cam[5 * row + c] = B.kf_cam[5 * (size_t)kf + c];
    O.fixed[row] = fixed;
}

// ------------------------------------------------------------------ 1. clear

__global__ __launch_bounds__(kThreads) void lg_clear_kernel(GWork V, int n_kf, int n_pt) {
    const int k = blockIdx.x;
    const size_t okf = kf_base(k, n_kf), opt = pt_base(k, n_pt);
    const int step = gridDim.y * kThreads;
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < n_pt; i += step) V.key[opt + i] = kNoKey;
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < n_kf; i += step) {
        V.fkey[okf + i] = kNoSight;
        V.kfkey[okf + i] = kNoKey;
        V.kfmark[okf + i] = kUnmarked;
        V.cnt[okf + i] = 0;
    }
}

// ------------------------------------------------------------------ 2. the local keyframes

__global__ __launch_bounds__(kThreads) void lg_locals_kernel(const orbgpu_localba_gather_job* __restrict__ jobs,
                                                             orbgpu_map_mirror M, orbgpu_map_mirror_ba B, GWork V) {
    __shared__ int s_wave[kWaves];
    __shared__ long long s_red[kWaves];
    __shared__ int s_bad, s_pk, s_off, s_nc;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    GState& S = V.st[k];
    if (tid == 0) {
        const int pk = jobs[k].kf;
        int bad = 0, off = 0, nc = 0;
        if (!in_range(pk, M.n_kf)) {
            bad = 1;
        } else {
            off = B.covis_all_offset[pk];
            nc = B.n_covis_all[pk];
            if (!span_ok(off, nc, B.n_covis_all_total)) bad = 1;
        }
        s_bad = bad, s_pk = pk, s_off = off, s_nc = bad ? 0 : nc;
        S.status = kPending;
        S.bad = S.skip = 0;
        S.n_local = S.n_points = S.n_mono = S.n_fixed = S.n_edges = 0;
    }
    __syncthreads();
    const size_t okf = kf_base(k, M.n_kf);
    unsigned* kfkey = V.kfkey + okf;
    int* kfmark = V.kfmark + okf;
    int* list = V.list + okf;
    const int pk = s_pk, off = s_off, nc = s_nc;
    int n_local = 0;
    long long slots = 0;
    const bool bad_kf = s_bad != 0;  // read by every thread before any of them raises s_bad below
    __syncthreads();
    if (!bad_kf) {
        // vNeighKFs (:548-555): the first occurrence of every keyframe, pKF before all of them
        if (tid == 0) atomicMin(&kfkey[pk], 0u);
        for (int i = tid; i < nc; i += kThreads) {
            const int c = B.covis_all[off + i];
            if (!in_range(c, M.n_kf)) atomicOr(&s_bad, 1);
            else atomicMin(&kfkey[c], (unsigned)i + 1u);
        }
        __syncthreads();
        if (tid == 0) {
            list[0] = pk;  // :544, not tested for isBad()
            kfmark[pk] = 0;
        }
        int base = 1;
        for (int s = 0; s < nc; s += kThreads) {
            const int i = s + tid;
            int c = -1;
            bool first = false;
            if (i < nc) {
                c = B.covis_all[off + i];
                first = in_range(c, M.n_kf) &&
                        __hip_atomic_load(&kfkey[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)i + 1u;
            }
            const bool listed = first && !M.kf_bad[c];
            const int pos = compact_slot(listed, lane, wave, s_wave, base);
            if (first) kfmark[c] = listed ? pos : kUnlisted;  // marked either way (:552)
            if (listed) list[pos] = c;                        // distinct keyframes: pos < n_kf
            compact_advance<kThreads>(s_wave, base);
            __syncthreads();
        }
        n_local = base;
    }
    __syncthreads();
    const bool bad_covis = s_bad != 0;
    __syncthreads();
    if (!bad_covis) {
        // the slots before each list position: numbers every (position, slot) in the walk's order
        bool bad = false;
        for (int s = 0; s < n_local; s += kThreads) {
            const int i = s + tid;
            long long c = 0;
            if (i < n_local) {
                const int kf = list[i];
                const int so = M.slot_offset[kf], ns = M.n_slots[kf];
                if (!span_ok(so, ns, M.n_slots_total)) bad = true;
                else c = ns;
            }
            const long long pre = stripe_prefix(c, slots, s_red);
            if (i < n_local) V.kfbase[okf + i] = (int)min(pre, 0x7fffffffLL);
        }
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
    }
    if (tid == 0) {
        if (s_bad) S.status = ORBGPU_LOCALBA_MAP_BAD_JOB;
        S.n_local = s_bad ? 0 : n_local;
        S.skip = slots >= (long long)ORBGPU_LOCALBA_MAP_MAX_SLOTS;
    }
}

// ------------------------------------------------------------------ 3-5. the local points

__device__ __forceinline__ bool walks_points(const GState& S) { return S.status == kPending && !S.skip; }

__global__ __launch_bounds__(kThreads) void lg_mark_kernel(orbgpu_map_mirror M, GWork V) {
    const int k = blockIdx.x, tid = threadIdx.x;
    GState& S = V.st[k];
    if (!walks_points(S)) return;
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    bool bad = false;
    for (int pos = blockIdx.y; pos < S.n_local; pos += gridDim.y) {
        const int kf = V.list[okf + pos];
        const int off = M.slot_offset[kf], ns = M.n_slots[kf];
        const unsigned g0 = (unsigned)V.kfbase[okf + pos];
        for (int s = tid; s < ns; s += kThreads) {
            const int id = M.slots[off + s];
            if (id == -1) continue;
            if (!in_range(id, M.n_pt)) bad = true;
            else if ((M.pt_flags[id] & ORBGPU_PT_VALID) && V.key[opt + id] > g0 + (unsigned)s)  // a stale read only costs an atomic
                atomicMin(&V.key[opt + id], g0 + (unsigned)s);
        }
    }
    if (bad) S.bad = 1;
}

// whether slot number g is its point's first occurrence; id is checked
__device__ __forceinline__ bool first_seen(const orbgpu_map_mirror& M, const unsigned* key, int id, unsigned g) {
    return in_range(id, M.n_pt) && key[id] == g;
}

__global__ __launch_bounds__(kThreads) void lg_count_kernel(orbgpu_map_mirror M, GWork V) {
    __shared__ long long s_red[kWaves];
    const int k = blockIdx.x, tid = threadIdx.x;
    GState& S = V.st[k];
    if (!walks_points(S) || S.bad) return;
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    const int n_local = S.n_local;
    for (int pos = blockIdx.y; pos < n_local; pos += gridDim.y) {
        const int kf = V.list[okf + pos];
        const int off = M.slot_offset[kf], ns = M.n_slots[kf];
        const unsigned g0 = (unsigned)V.kfbase[okf + pos];
        int c = 0;
        for (int s = tid; s < ns; s += kThreads) c += first_seen(M, V.key + opt, M.slots[off + s], g0 + (unsigned)s);
        const long long t = block_sum(c, s_red);
        if (tid == 0 && t) {
            V.cnt[okf + pos] = (int)t;
            atomicAdd(&S.n_points, (int)t);  // distinct points: the sum is at most n_pt
        }
    }
}

__global__ __launch_bounds__(kThreads) void lg_points_kernel(orbgpu_map_mirror M, GWork V) {
    __shared__ long long s_red[kWaves];
    __shared__ int s_wave[kWaves];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GState& S = V.st[k];
    if (!walks_points(S) || S.bad) return;
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    const int n_local = S.n_local;
    for (int pos = blockIdx.y; pos < n_local; pos += gridDim.y) {
        if (V.cnt[okf + pos] == 0) continue;
        long long before = 0;  // the first occurrences in the keyframes before this one
        for (int i = tid; i < pos; i += kThreads) before += V.cnt[okf + i];
        before = block_sum(before, s_red);
        const int kf = V.list[okf + pos];
        const int off = M.slot_offset[kf], ns = M.n_slots[kf];
        const unsigned g0 = (unsigned)V.kfbase[okf + pos];
        int base = 0;
        for (int s0 = 0; s0 < ns; s0 += kThreads) {
            const int s = s0 + tid;
            const int id = s < ns ? M.slots[off + s] : -1;
            const bool ok = s < ns && first_seen(M, V.key + opt, id, g0 + (unsigned)s);
            const int r = compact_slot(ok, lane, wave, s_wave, base);
            if (ok) V.ptlist[opt + before + r] = id;  // distinct points: before + r < n_pt
            compact_advance<kThreads>(s_wave, base);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ 6-7. the fixed cameras, the edge counts

__device__ __forceinline__ unsigned long long sight(int idx, int o) {
    return ((unsigned long long)(unsigned)idx << 32) | (unsigned)o;
}

__global__ __launch_bounds__(kThreads) void lg_sight_kernel(orbgpu_map_mirror M, orbgpu_map_mirror_ba B, GWork V) {
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    GState& S = V.st[k];
    if (!walks_points(S) || S.bad) return;
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    const int n_points = S.n_points;
    bool bad = false;
    int n_mono = 0;
    for (int idx = blockIdx.y * kWaves + wave; idx < n_points; idx += gridDim.y * kWaves) {
        const int id = V.ptlist[opt + idx];
        const int off = M.obs_offset[id], c = M.n_obs[id];
        int ne = 0;
        if (!span_ok(off, c, M.n_obs_total)) {
            bad = true;
        } else {
            for (int o0 = 0; o0 < c; o0 += 64) {
                const int o = o0 + lane;
                bool edge = false, mono = false;
                if (o < c) {
                    const int kf = M.obs[off + o];
                    if (!in_range(kf, M.n_kf)) {
                        bad = true;
                    } else {
                        if (V.kfmark[okf + kf] == kUnmarked) atomicMin(&V.fkey[okf + kf], sight(idx, o));  // :590-592
                        if (!M.kf_bad[kf]) {  // :688
                            const int oi = B.obs_idx[off + o], so = M.slot_offset[kf], ns = M.n_slots[kf];
                            if (!span_ok(so, ns, M.n_slots_total) || !in_range(oi, ns)) {
                                bad = true;
                            } else {
                                edge = true;
                                mono = B.kp_obs[3 * ((size_t)so + oi) + 2] < 0.f;  // :693
                            }
                        }
                    }
                }
                ne += __popcll(__ballot(edge));
                n_mono += __popcll(__ballot(mono));
            }
        }
        if (lane == 0) V.ecnt[opt + idx] = ne;
    }
    if (bad) S.bad = 1;
    if (lane == 0 && n_mono) atomicAdd(&S.n_mono, n_mono);
}

// whether observation o of local point idx is the first sight of a fixed camera that is listed
__device__ __forceinline__ bool lists_fixed(const orbgpu_map_mirror& M, const GWork& V, size_t okf, int kf, int idx, int o) {
    return V.kfmark[okf + kf] == kUnmarked && V.fkey[okf + kf] == sight(idx, o) && !M.kf_bad[kf];  // :590-594
}

__global__ __launch_bounds__(kThreads) void lg_fixed_kernel(orbgpu_map_mirror M, GWork V) {
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GState& S = V.st[k];
    if (!walks_points(S) || S.bad) return;  // every id below was checked by lg_sight_kernel
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    const int n_points = S.n_points;
    for (int idx = blockIdx.y * kWaves + wave; idx < n_points; idx += gridDim.y * kWaves) {
        const int id = V.ptlist[opt + idx];
        const int off = M.obs_offset[id], c = M.n_obs[id];
        int nf = 0;
        for (int o0 = 0; o0 < c; o0 += 64) {
            const int o = o0 + lane;
            nf += __popcll(__ballot(o < c && lists_fixed(M, V, okf, M.obs[off + o], idx, o)));
        }
        if (lane == 0) V.fcnt[opt + idx] = nf;
    }
}

// ------------------------------------------------------------------ 8. the sums, the status, the local poses

__global__ __launch_bounds__(kThreads) void lg_finish_kernel(orbgpu_map_mirror M, orbgpu_map_mirror_ba B, Dims D,
                                                             GWork V, Out O) {
    __shared__ long long s_red[kWaves];
    const int k = blockIdx.x, tid = threadIdx.x;
    GState& S = V.st[k];
    orbgpu_localba_gather_result& R = O.results[k];
    orbgpu_localba_job& L = O.ba_jobs[k];
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    int status = S.status;
    if (status == kPending && S.bad) status = ORBGPU_LOCALBA_MAP_BAD_JOB;
    long long n_edges = 0, n_fixed = 0;
    const int n_local = S.n_local, n_points = (status == kPending && !S.skip) ? S.n_points : 0;
    if (status == kPending) {
        for (int s = 0; s < n_points; s += kThreads) {
            const int i = s + tid;
            const long long e = i < n_points ? V.ecnt[opt + i] : 0, f = i < n_points ? V.fcnt[opt + i] : 0;
            const long long eb = stripe_prefix(e, n_edges, s_red), fb = stripe_prefix(f, n_fixed, s_red);
            if (i < n_points) {
                V.ebase[opt + i] = (int)min(eb, 0x7fffffffLL);
                V.fbase[opt + i] = (int)fb;  // distinct keyframes: below n_kf
            }
        }
        if (n_edges > 0x7fffffffLL) status = ORBGPU_LOCALBA_MAP_BAD_JOB;  // more edges than obs[] holds: spans overlap
    }
    if (status == kPending) {
        const bool over = S.skip || n_local > D.kf_stride || (long long)n_local + n_fixed > D.pose_stride ||
                          n_points > D.point_stride || n_edges > D.edge_stride;
        status = over ? ORBGPU_LOCALBA_MAP_CAPACITY : ORBGPU_LOCALBA_MAP_OK;
        for (int i = tid; i < n_local; i += kThreads) {
            const int kf = V.list[okf + i];
            if (i < D.kf_stride) O.local_kfs[(size_t)k * D.kf_stride + i] = kf;
            if (i < D.pose_stride) copy_pose(O, B, (size_t)k * D.pose_stride + i, kf, B.kf_first[kf] ? 1 : 0);  // :624
        }
    }
    if (tid == 0) {
        const bool ok = status == ORBGPU_LOCALBA_MAP_OK, counted = status != ORBGPU_LOCALBA_MAP_BAD_JOB;
        S.status = status;
        S.n_fixed = counted ? (int)n_fixed : 0;
        S.n_edges = counted ? (int)n_edges : 0;
        R.status = status;
        R.n_local = counted ? n_local : 0;
        R.n_fixed = S.n_fixed;
        R.n_points = counted ? n_points : 0;
        R.n_edges = S.n_edges;
        R.n_mono = counted && !S.skip ? S.n_mono : 0;
        R.n_stereo = R.n_edges - R.n_mono;
        R.pad = 0;
        L.n_poses = ok ? n_local + (int)n_fixed : -1;
        L.n_local = ok ? n_local : -1;
        L.n_points = ok ? n_points : -1;
        L.n_edges = ok ? (int)n_edges : -1;
        L.pose_offset = k * D.pose_stride;  // n * stride fits an int: checked on the host
        L.point_offset = k * D.point_stride;
        L.edge_offset = k * D.edge_stride;
        L.out_pose_offset = k * D.kf_stride;
    }
}

// ------------------------------------------------------------------ 9-10. the fixed cameras, the points, the edges

__device__ __forceinline__ bool places(const GState& S) {
    return (S.status == ORBGPU_LOCALBA_MAP_OK || S.status == ORBGPU_LOCALBA_MAP_CAPACITY) && !S.skip;
}

__global__ __launch_bounds__(kThreads) void lg_place_kernel(orbgpu_map_mirror M, orbgpu_map_mirror_ba B, Dims D, GWork V,
                                                            Out O) {
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GState& S = V.st[k];
    if (!places(S)) return;
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    const int n_points = S.n_points, n_local = S.n_local;
    for (int idx = blockIdx.y * kWaves + wave; idx < n_points; idx += gridDim.y * kWaves) {
        const int id = V.ptlist[opt + idx];
        if (idx < D.point_stride) {
            const size_t row = (size_t)k * D.point_stride + idx;
            if (lane < 3) O.Xw[3 * row + lane] = M.pos[3 * (size_t)id + lane];
            if (lane == 3) O.local_points[row] = id;
        }
        if (V.fcnt[opt + idx] == 0) continue;
        const int off = M.obs_offset[id], c = M.n_obs[id];
        int before = V.fbase[opt + idx];
        for (int o0 = 0; o0 < c; o0 += 64) {
            const int o = o0 + lane;
            const int kf = o < c ? M.obs[off + o] : -1;
            const bool ok = o < c && lists_fixed(M, V, okf, kf, idx, o);
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int fp = before + (int)__popcll(m & ((1ull << lane) - 1));
                const long long p = (long long)n_local + fp;  // the vertices' order (:618-642)
                V.fpos[okf + kf] = (int)min(p, 0x7fffffffLL);
                if (p < D.pose_stride) {
                    O.fixed_kfs[(size_t)k * D.pose_stride + fp] = kf;
                    copy_pose(O, B, (size_t)k * D.pose_stride + p, kf, 1);  // :638
                }
            }
            before += (int)__popcll(m);
        }
    }
}

__global__ __launch_bounds__(kThreads) void lg_edges_kernel(orbgpu_map_mirror M, orbgpu_map_mirror_ba B, Dims D, GWork V,
                                                            Out O) {
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GState& S = V.st[k];
    if (!places(S) || S.n_edges == 0) return;
    const size_t okf = kf_base(k, M.n_kf), opt = pt_base(k, M.n_pt);
    const int n_points = S.n_points;
    for (int idx = blockIdx.y * kWaves + wave; idx < n_points; idx += gridDim.y * kWaves) {
        if (V.ecnt[opt + idx] == 0) continue;
        const int id = V.ptlist[opt + idx];
        const int off = M.obs_offset[id], c = M.n_obs[id];
        long long before = V.ebase[opt + idx];
        for (int o0 = 0; o0 < c && before < D.edge_stride; o0 += 64) {
            const int o = o0 + lane;
            const int kf = o < c ? M.obs[off + o] : -1;
            const bool ok = o < c && !M.kf_bad[kf];  // :688
            const unsigned long long m = __ballot(ok);
            const long long e = before + (long long)__popcll(m & ((1ull << lane) - 1));
            if (ok && e < D.edge_stride) {
                const int oi = B.obs_idx[off + o];  // mit->second (:690), checked by lg_sight_kernel
                const size_t kp = (size_t)M.slot_offset[kf] + oi, row = (size_t)k * D.edge_stride + e;
                const int mark = V.kfmark[okf + kf];
                const float ur = B.kp_obs[3 * kp + 2];
                O.edge_pose[row] = mark >= 0 ? mark : V.fpos[okf + kf];
                O.edge_point[row] = idx;
                O.obs[3 * row] = B.kp_obs[3 * kp];
                O.obs[3 * row + 1] = B.kp_obs[3 * kp + 1];
                O.obs[3 * row + 2] = ur < 0.f ? -1.0f : ur;
                O.inv_sigma2[row] = B.kp_inv_sigma2[kp];
                O.edge_kf[row] = kf;
                O.edge_slot[row] = oi;
            }
            before += (long long)__popcll(m);
        }
    }
}

// ------------------------------------------------------------------ the collection

struct Collect {
    const orbgpu_localba_job* ba_jobs;
    const float* obs;
    const int* edge_point;
    const int* local_kfs;
    const int* local_points;
    const int* edge_kf;
    const int* edge_slot;
    const uint8_t* erase;
    const float* Tcw_out;
    const float* Xw_out;
    int* to_erase;
    int* n_erase;
    float* kf_Tcw;
    float* pos;
    int n_kf, n_pt;
};

// a gathered job: counts that are not negative and within the strides
__device__ __forceinline__ bool gathered(const orbgpu_localba_job& j, const Dims& D) {
    return j.n_local >= 0 && j.n_local <= D.kf_stride && j.n_points >= 0 && j.n_points <= D.point_stride &&
           j.n_edges >= 0 && j.n_edges <= D.edge_stride;
}

__global__ __launch_bounds__(kThreads) void lc_erase_kernel(Collect C, Dims D) {
    __shared__ int s_wave[kWaves];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const orbgpu_localba_job j = C.ba_jobs[k];
    if (!gathered(j, D)) {
        if (tid == 0) C.n_erase[k] = 0;
        return;
    }
    const size_t eo = (size_t)k * D.edge_stride, lo = (size_t)k * D.point_stride;
    int base = 0;
    for (int cls = 0; cls < 2; ++cls) {  // vpEdgesMono (:818-832), then vpEdgesStereo (:834-847)
        for (int s = 0; s < j.n_edges; s += kThreads) {
            const int e = s + tid;
            bool ok = false;
            int pt = -1;
            if (e < j.n_edges && C.erase[eo + e]) {
                pt = C.edge_point[eo + e];
                ok = in_range(pt, j.n_points) && (C.obs[3 * (eo + e) + 2] < 0.f) == (cls == 0);
            }
            const int r = compact_slot(ok, lane, wave, s_wave, base);
            if (ok) {
                int* t = C.to_erase + 3 * (eo + r);  // r < n_edges <= edge_stride
                t[0] = C.edge_kf[eo + e];
                t[1] = C.local_points[lo + pt];
                t[2] = C.edge_slot[eo + e];
            }
            compact_advance<kThreads>(s_wave, base);
            __syncthreads();
        }
    }
    if (tid == 0) C.n_erase[k] = base;
}

__global__ __launch_bounds__(kThreads) void lc_write_kernel(Collect C, Dims D) {
    const int k = blockIdx.x;
    const orbgpu_localba_job j = C.ba_jobs[k];
    if (!gathered(j, D)) return;
    const int step = gridDim.y * kThreads, t0 = blockIdx.y * kThreads + threadIdx.x;
    if (C.kf_Tcw)  // SetPose (:866-870)
        for (int i = t0; i < 12 * j.n_local; i += step) {
            const size_t row = (size_t)k * D.kf_stride + i / 12;
            const int kf = C.local_kfs[row];
            if (in_range(kf, C.n_kf)) C.kf_Tcw[12 * (size_t)kf + i % 12] = C.Tcw_out[16 * row + i % 12];
        }
    if (C.pos)  // SetWorldPos (:876-882)
        for (int i = t0; i < 3 * j.n_points; i += step) {
            const size_t row = (size_t)k * D.point_stride + i / 3;
            const int id = C.local_points[row];
            if (in_range(id, C.n_pt)) C.pos[3 * (size_t)id + i % 3] = C.Xw_out[3 * row + i % 3];
        }
}

bool fits_int(long long a, long long b) { return a * b <= 0x7fffffffLL; }

int grid_y(long long items) {
    const long long g = items < 1 ? 1 : items;
    return (int)(g < kMaxGridY ? g : kMaxGridY);
}

// what the gather reads of the two mirrors
const char* mirrors_error(const orbgpu_map_mirror* m, const orbgpu_map_mirror_ba* b) {
    if (!m || !b) return "mirror or mirror_ba is NULL";
    if (m->n_kf < 0 || m->n_pt < 0 || m->n_slots_total < 0 || m->n_obs_total < 0 || b->n_covis_all_total < 0)
        return "a mirror count is negative";
    if (m->n_kf > 0 && (!m->kf_bad || !m->slot_offset || !m->n_slots || !b->covis_all_offset || !b->n_covis_all ||
                        !b->kf_first || !b->kf_Tcw || !b->kf_cam))
        return "a keyframe array of the mirrors is NULL";
    if (m->n_pt > 0 && (!m->pt_flags || !m->obs_offset || !m->n_obs || !m->pos)) return "a point array of the mirror is NULL";
    if (m->n_slots_total > 0 && (!m->slots || !b->kp_obs || !b->kp_inv_sigma2)) return "slots, kp_obs or kp_inv_sigma2 is NULL";
    if (m->n_obs_total > 0 && (!m->obs || !b->obs_idx)) return "obs or obs_idx is NULL";
    if (b->n_covis_all_total > 0 && !b->covis_all) return "covis_all is NULL";
    return nullptr;
}

const char* strides_error(int n, int kf_stride, int pose_stride, int point_stride, int edge_stride) {
    if (n < 0) return "n is negative";
    if (kf_stride <= 0 || pose_stride <= 0 || point_stride <= 0 || edge_stride <= 0) return "a stride is not positive";
    if (!fits_int(n, 16LL * kf_stride) || !fits_int(n, 12LL * pose_stride) || !fits_int(n, 3LL * point_stride) ||
        !fits_int(n, 3LL * edge_stride))
        return "n times a stride overflows";
    return nullptr;
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

size_t orbgpu_local_ba_gather_workspace_bytes(int n, int n_kf, int n_pt) {
    const long long N = n > 0 ? n : 1;
    if (!fits_int(N, n_kf > 0 ? n_kf : 1) || !fits_int(N, n_pt > 0 ? n_pt : 1)) return 0;
    size_t bytes = 0;
    carve(nullptr, n, n_kf, n_pt, &bytes);
    return bytes;
}

int orbgpu_local_ba_gather_batch_device(int n, const orbgpu_localba_gather_job* d_jobs,
                                        const orbgpu_map_mirror* mirror, const orbgpu_map_mirror_ba* mirror_ba,
                                        int kf_stride, int pose_stride, int point_stride, int edge_stride,
                                        void* d_workspace, orbgpu_localba_gather_result* d_results,
                                        orbgpu_localba_job* d_ba_jobs, float* d_Tcw, uint8_t* d_fixed, float* d_cam,
                                        float* d_Xw, int* d_edge_pose, int* d_edge_point, float* d_obs,
                                        float* d_inv_sigma2, int* d_local_kfs, int* d_fixed_kfs, int* d_local_points,
                                        int* d_edge_kf, int* d_edge_slot, void* stream) {
    if (const char* e = strides_error(n, kf_stride, pose_stride, point_stride, edge_stride)) return fail(ORBGPU_ERR_ARG, e);
    if (n > 0 && (!d_jobs || !d_workspace || !d_results || !d_ba_jobs || !d_Tcw || !d_fixed || !d_cam || !d_Xw ||
                  !d_edge_pose || !d_edge_point || !d_obs || !d_inv_sigma2 || !d_local_kfs || !d_fixed_kfs ||
                  !d_local_points || !d_edge_kf || !d_edge_slot))
        return fail(ORBGPU_ERR_ARG, "a NULL pointer with n > 0");
    if (n > 0 || mirror || mirror_ba)
        if (const char* e = mirrors_error(mirror, mirror_ba)) return fail(ORBGPU_ERR_ARG, e);
    if (n > 0 && orbgpu_local_ba_gather_workspace_bytes(n, mirror->n_kf, mirror->n_pt) == 0)
        return fail(ORBGPU_ERR_ARG, "n * n_kf or n * n_pt overflows");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const orbgpu_map_mirror M = *mirror;
    const orbgpu_map_mirror_ba B = *mirror_ba;
    const Dims D{kf_stride, pose_stride, point_stride, edge_stride};
    const GWork V = carve(d_workspace, n, M.n_kf, M.n_pt, nullptr);
    const Out O{d_results, d_ba_jobs, d_Tcw,       d_fixed,     d_cam,          d_Xw,      d_edge_pose, d_edge_point,
                d_obs,     d_inv_sigma2, d_local_kfs, d_fixed_kfs, d_local_points, d_edge_kf, d_edge_slot};
    const dim3 block(kThreads), per_job(n), per_kf(n, grid_y(M.n_kf)),
        per_point(n, grid_y(((long long)M.n_pt + kWaves - 1) / kWaves));
    const int most = M.n_pt > M.n_kf ? M.n_pt : M.n_kf;
    hipLaunchKernelGGL(lg_clear_kernel, dim3(n, grid_y(((long long)most + kThreads - 1) / kThreads)), block, 0, s, V, M.n_kf,
                       M.n_pt);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_locals_kernel, per_job, block, 0, s, d_jobs, M, B, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_mark_kernel, per_kf, block, 0, s, M, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_count_kernel, per_kf, block, 0, s, M, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_points_kernel, per_kf, block, 0, s, M, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_sight_kernel, per_point, block, 0, s, M, B, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_fixed_kernel, per_point, block, 0, s, M, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_finish_kernel, per_job, block, 0, s, M, B, D, V, O);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_place_kernel, per_point, block, 0, s, M, B, D, V, O);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lg_edges_kernel, per_point, block, 0, s, M, B, D, V, O);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

int orbgpu_local_ba_collect_batch_device(int n, const orbgpu_localba_job* d_ba_jobs, int kf_stride, int point_stride,
                                         int edge_stride, const float* d_obs, const int* d_edge_point,
                                         const int* d_local_kfs, const int* d_local_points, const int* d_edge_kf,
                                         const int* d_edge_slot, const uint8_t* d_erase, const float* d_Tcw_out,
                                         const float* d_Xw_out, int* d_to_erase, int* d_n_erase, int n_kf, int n_pt,
                                         float* d_kf_Tcw, float* d_pos, void* stream) {
    if (const char* e = strides_error(n, kf_stride, 1, point_stride, edge_stride)) return fail(ORBGPU_ERR_ARG, e);
    if (n_kf < 0 || n_pt < 0) return fail(ORBGPU_ERR_ARG, "n_kf or n_pt is negative");
    if (n > 0 && (!d_ba_jobs || !d_obs || !d_edge_point || !d_local_kfs || !d_local_points || !d_edge_kf ||
                  !d_edge_slot || !d_erase || !d_to_erase || !d_n_erase))
        return fail(ORBGPU_ERR_ARG, "a NULL pointer with n > 0");
    if (n > 0 && ((d_kf_Tcw && !d_Tcw_out) || (d_pos && !d_Xw_out)))
        return fail(ORBGPU_ERR_ARG, "a mirror array to write without the outputs to write it from");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const Dims D{kf_stride, 1, point_stride, edge_stride};
    const Collect C{d_ba_jobs, d_obs,    d_edge_point, d_local_kfs, d_local_points, d_edge_kf, d_edge_slot, d_erase,
                    d_Tcw_out, d_Xw_out, d_to_erase,   d_n_erase,   d_kf_Tcw,       d_pos,     n_kf,        n_pt};
    hipLaunchKernelGGL(lc_erase_kernel, dim3(n), dim3(kThreads), 0, s, C, D);
    ORB_HIP(hipGetLastError());
    if (d_kf_Tcw || d_pos) {
        const long long items = 12LL * kf_stride > 3LL * point_stride ? 12LL * kf_stride : 3LL * point_stride;
        hipLaunchKernelGGL(lc_write_kernel, dim3(n, grid_y((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, C, D);
        ORB_HIP(hipGetLastError());
    }
    return ORBGPU_OK;
}

}  // extern "C"
