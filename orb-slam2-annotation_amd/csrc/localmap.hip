// localmap.hip -- Tracking::UpdateLocalMap on the device (include/orbgpu_localmap.h): the
// step between the two halves of track.hip, batched over independent frames.  It reads call 1's
// rows and a mirror of the map in HBM and writes call 2's point table, frame_mp and job.
//
//  orbgpu_update_local_map_batch_device (src/Tracking.cpp:1571-1745), seven launches:
//    1 lm_clear_kernel    (chunk, job)   the job's vote, mark and key arrays in the workspace
//    2 lm_vote_kernel     (job)          the job's checks; the held points vote over their
//                                        observations (atomic add), bad ones are counted as nulled;
//                                        "in row 0" / "in row 1" marks per mirror point (atomic or)
//    3 lm_walk_kernel     (job)          K1 by a prefix sum in rank order and the first strict
//                                        maximum; the K2 walk's candidates staged in LDS by the block,
//                                        the walk itself on one wave (:1682-1736), or the
//                                        previous list when nobody voted (:1646); the exclusive sum
//                                        of the list's slot counts, which numbers every (list
//                                        position, slot) pair
//    4 lm_mark_kernel     (keyframe, job) atomic min of that number over each good point's slots:
//                                        its first occurrence (:1594-1614)
//    5 lm_count_kernel    (keyframe, job) the first occurrences per keyframe
//    6 lm_scatter_kernel  (keyframe, job) the keyframe's base = the sum of the counts before it;
//                                        first occurrences compacted in slot order; local_points and
//                                        the table entry gathered from the mirror
//    7 lm_finish_kernel   (job)          frame_mp, the frame-held extras (deduplicated in LDS, in
//                                        keypoint order), local_kfs, the result, the prepared job
//
// Votes and marks are integer atomics, exact in any order; positions come from prefix sums in key
// order, so every output byte is a function of the job and the mirror.  No launch waits for
// another workgroup; nothing synchronises with the host.  Every id read from the job or the mirror
// is range-checked before it is used as an index: a job with one out of range ends as BAD_JOB and
// writes nothing but its result (all output is written by launches 6 and 7, after the last check).
#include "../../include/orbgpu_localmap.h"
#include "host_common.h"
#include "ransac_device.h"

namespace orbgpu {

namespace {

using namespace ransacdev;

constexpr int kThreads = 256;
constexpr int kVoteThreads = 1024;  // lm_vote_kernel: a keypoint per thread, the chain of loads is what it waits for
constexpr int kMaxKps = 4096;  // proj_kernel's keypoint capacity, as track.hip
constexpr int kCovis = ORBGPU_LOCALMAP_COVIS;
constexpr int kMaxKfs = ORBGPU_LOCALMAP_MAX_KFS;
constexpr int kWalkList = kMaxKfs + 4;  // the walk appends at most 3 to a list of at most 80
constexpr int kCandidates = 32;  // what the walk can read of one K1 member: 10 covisibles, the parent, 21 children
constexpr int kStagedChildren = kCandidates - kCovis - 1;
constexpr int kBadId = -2;  // a staged id outside the mirror
constexpr unsigned kNoKey = 0xffffffffu;
constexpr unsigned kInRow0 = 1u, kInRow1 = 2u;

enum { kPending = -1, kOverflow = -2 };  // kOverflow: CAPACITY before any point was gathered

struct MState {  // a job between the launches
    int status;  // kPending, kOverflow or ORBGPU_LOCALMAP_BAD_JOB
    int kept;
    int n_k1;
    int n_list;  // mvpLocalKeyFrames.size(), the true one
    int ref_kf;
    int n_nulled;
    int bad_slot;  // written by lm_mark_kernel only: a slot id out of range
    int pad;
};

struct MWork {  // the opaque block, carved
    MState* st;
    int* votes;     // per job and keyframe
    int* kfpos;     // per job and keyframe: the K1 position or -1 (mnTrackReferenceForFrame)
    unsigned* key;  // per job and point: the number of its first (list position, slot), or kNoKey
    unsigned* pm;   // per job and point: kInRow0 | kInRow1
    int* tix;       // per job and local point: its table index
    int* list;      // per job: the local keyframes, kf_stride
    int* kfbase;    // per job and list position: the slots before it
    int* cnt;       // per job and list position: first occurrences
};

inline MWork carve(void* base, int n, int kf_stride, int n_kf, int n_pt, size_t* bytes) {
    const size_t N = (size_t)(n > 0 ? n : 1), K = (size_t)(kf_stride > 0 ? kf_stride : 1),
                 NK = (size_t)(n_kf > 0 ? n_kf : 1), NP = (size_t)(n_pt > 0 ? n_pt : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    MWork v;
    v.st = take<MState>(p, N);
    v.votes = take<int>(p, N * NK);
    v.kfpos = take<int>(p, N * NK);
    v.key = take<unsigned>(p, N * NP);
    v.pm = take<unsigned>(p, N * NP);
    v.tix = take<int>(p, N * NP);
    v.list = take<int>(p, N * K);
    v.kfbase = take<int>(p, N * K);
    v.cnt = take<int>(p, N * K);
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return v;
}

struct Dims {
    int stride, point_stride, kf_stride;
};

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

// offset + count within an array of `total`
__device__ __forceinline__ bool span_ok(int off, int cnt, int total) {
    return off >= 0 && cnt >= 0 && (long long)off + cnt <= (long long)total;
}

// the sum of v over the block; every thread calls it, s_red holds kThreads / 64 values
__device__ __forceinline__ long long block_sum(long long v, long long* s_red) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();  // s_red may still be read from the call before
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int w = 0; w < kThreads / 64; ++w) t += s_red[w];
    return t;
}

// ------------------------------------------------------------------ 1. clear

__global__ __launch_bounds__(kThreads) void lm_clear_kernel(MWork V, int n_kf, int n_pt, int kf_stride) {
    const int k = blockIdx.x;
    const size_t okf = (size_t)k * (n_kf > 0 ? n_kf : 1), opt = (size_t)k * (n_pt > 0 ? n_pt : 1),
                 ol = (size_t)k * kf_stride;
    const int step = gridDim.y * kThreads;
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < n_pt; i += step) {
        V.key[opt + i] = kNoKey;
        V.pm[opt + i] = 0u;
    }
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < n_kf; i += step) {
        V.votes[okf + i] = 0;
        V.kfpos[okf + i] = -1;
    }
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < kf_stride; i += step) V.cnt[ol + i] = 0;
}

// ------------------------------------------------------------------ 2. the votes

__global__ __launch_bounds__(kVoteThreads) void lm_vote_kernel(const orbgpu_update_local_map_job* __restrict__ jobs,
                                                           orbgpu_map_mirror M, Dims D, MWork V) {
    __shared__ int s_status, s_bad, s_nulled;
    const int k = blockIdx.x, tid = threadIdx.x;
    const orbgpu_update_local_map_job& J = jobs[k];
    if (tid == 0) {
        int status = kPending;
        if (J.n_kp < 0 || J.src_n < 0 || J.n_prev_kfs < 0 || (J.n_kp > 0 && !J.rows) || (J.src_n > 0 && !J.src_pt_id) ||
            (J.n_prev_kfs > 0 && !J.prev_kfs) || !J.out_flags || !J.out_pos || !J.out_normal || !J.out_desc ||
            !J.out_min_dist || !J.out_max_dist || !J.frame_mp || !J.local_job)
            status = ORBGPU_LOCALMAP_BAD_JOB;
        else if (J.n_kp > min(D.stride, kMaxKps))
            status = kOverflow;
        s_status = status;
        s_bad = s_nulled = 0;
    }
    __syncthreads();
    int status = s_status;
    if (status == kPending) {
        const size_t okf = (size_t)k * (M.n_kf > 0 ? M.n_kf : 1), opt = (size_t)k * (M.n_pt > 0 ? M.n_pt : 1);
        const int* row0 = J.rows;
        const int* row1 = J.rows + D.stride;
        int nulled = 0;
        bool bad = false;
        for (int j = tid; j < J.n_kp; j += kVoteThreads) {
            const int t0 = row0[j], t1 = row1[j];
            if (t0 >= 0) {  // before the cull: what call 1 matched
                const int id = t0 < J.src_n ? J.src_pt_id[t0] : -2;
                if (id < -1 || id >= M.n_pt) bad = true;
                else if (id >= 0) atomicOr(&V.pm[opt + id], kInRow0);
            }
            if (t1 < 0) continue;  // mvpMapPoints[j] is NULL
            const int id = t1 < J.src_n ? J.src_pt_id[t1] : -2;
            if (id < -1 || id >= M.n_pt) {
                bad = true;
                continue;
            }
            if (id < 0) {  // a temporal point: never bad, no observations; call 1's entry is its source
                if (!J.src_pos || !J.src_desc) bad = true;
                continue;
            }
            if (!(M.pt_flags[id] & ORBGPU_PT_VALID)) {  // :1641
                ++nulled;
                continue;
            }
            atomicOr(&V.pm[opt + id], kInRow1);
            const int off = M.obs_offset[id], c = M.n_obs[id];
            if (!span_ok(off, c, M.n_obs_total)) {
                bad = true;
                continue;
            }
            for (int o = 0; o < c; o += 4) {  // keyframeCounter[it->first]++ (:1637), four loads in flight
                int kf[4];
                for (int u = 0; u < 4; ++u) kf[u] = o + u < c ? M.obs[off + o + u] : -1;
                for (int u = 0; u < 4; ++u) {
                    if (o + u >= c) break;
                    if (!in_range(kf[u], M.n_kf)) bad = true;
                    else atomicAdd(&V.votes[okf + kf[u]], 1);
                }
            }
        }
        if (bad) atomicOr(&s_bad, 1);
        if (nulled) atomicAdd(&s_nulled, nulled);
        __syncthreads();
        if (s_bad) status = ORBGPU_LOCALMAP_BAD_JOB;
    }
    if (tid == 0) {
        MState& S = V.st[k];
        S.status = status;
        S.kept = 0;
        S.n_k1 = S.n_list = 0;
        S.ref_kf = -1;
        S.n_nulled = status == kPending ? s_nulled : 0;
        S.bad_slot = 0;
        S.pad = 0;
    }
}

// ------------------------------------------------------------------ 3. the keyframes

// c among the keyframes the walk appended, s_list[n_k1, n)
__device__ __forceinline__ bool appended(const int* s_list, int n_k1, int n, int c) {
    bool hit = false;
    for (int a = n_k1; a < n; ++a) hit |= s_list[a] == c;
    return hit;
}

__global__ __launch_bounds__(kThreads) void lm_walk_kernel(const orbgpu_update_local_map_job* __restrict__ jobs,
                                                           orbgpu_map_mirror M, Dims D, MWork V) {
    __shared__ int s_wave[kThreads / 64];
    __shared__ long long s_red[kThreads / 64];
    __shared__ unsigned long long s_best;
    __shared__ int s_any, s_bad, s_n;
    __shared__ int s_list[kWalkList];
    __shared__ int s_cand[kMaxKfs * kCandidates], s_nc[kMaxKfs];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    MState& S = V.st[k];
    if (S.status != kPending) return;
    const orbgpu_update_local_map_job& J = jobs[k];
    const size_t okf = (size_t)k * (M.n_kf > 0 ? M.n_kf : 1), ol = (size_t)k * D.kf_stride;
    int* list = V.list + ol;
    const int* votes = V.votes + okf;
    int* kfpos = V.kfpos + okf;
    if (tid == 0) {
        s_best = 0ull;
        s_any = s_bad = 0;
    }
    __syncthreads();
    // K1 (:1660-1676): the voted keyframes that are not bad, in rank order; pKFmax the first strict maximum
    int base = 0;
    for (int s = 0; s < M.n_kf; s += kThreads) {
        const int r = s + tid;
        int kf = -1, v = 0;
        if (r < M.n_kf) {
            kf = M.kf_by_rank ? M.kf_by_rank[r] : r;
            if (!in_range(kf, M.n_kf)) {
                atomicOr(&s_bad, 1);
                kf = -1;
            } else {
                v = votes[kf];
            }
        }
        if (v > 0) s_any = 1;
        const bool ok = v > 0 && !M.kf_bad[kf];
        const int pos = compact_slot(ok, lane, wave, s_wave, base);
        if (ok) {
            kfpos[kf] = pos;
            if (pos < D.kf_stride) list[pos] = kf;
            if (pos < kWalkList) s_list[pos] = kf;
            atomicMax(&s_best, ((unsigned long long)(unsigned)v << 32) | (unsigned)(0x7fffffff - r));
        }
        compact_advance<kThreads>(s_wave, base);
        __syncthreads();
    }
    const int n_k1 = base;
    const bool kept = !s_any;
    int n_list = n_k1;
    if (kept) {  // `return` at :1646: the previous list stands
        n_list = J.n_prev_kfs;
        for (int i = tid; i < n_list; i += kThreads) {
            const int kf = J.prev_kfs[i];
            if (!in_range(kf, M.n_kf)) atomicOr(&s_bad, 1);
            else if (i < D.kf_stride) list[i] = kf;
        }
    } else if (n_k1 > 0 && n_k1 <= kMaxKfs) {
        // The K2 walk (:1682-1736) visits the K1 members only, while the list holds at most 80.  What it can
        // read is known now, so the whole block stages it in two rounds of loads: per member the ten
        // covisibles, the parent and the first kStagedChildren children, each already -1 when it is bad (not
        // asked of the parent) or in K1, and kBadId when it lies outside the mirror, which counts only if the
        // walk gets to that member.
        for (int e = tid; e < n_k1 * kCandidates; e += kThreads) {
            const int kf = s_list[e / kCandidates], q = e % kCandidates;
            int c = -1;
            if (q < kCovis) {
                c = M.covis[(size_t)kf * kCovis + q];
                if (c < -1 || c >= M.n_kf) c = kBadId;
            } else if (q == kCovis) {
                c = M.parent[kf];
                if (c < -1 || c >= M.n_kf) c = kBadId;
            } else {
                const int coff = M.child_offset[kf], nc = M.n_children[kf], u = q - kCovis - 1;
                if (!span_ok(coff, nc, M.n_children_total)) {
                    c = kBadId;
                } else if (u < nc) {
                    c = M.children[coff + u];
                    if (!in_range(c, M.n_kf)) c = kBadId;
                }
                if (u == 0) s_nc[e / kCandidates] = span_ok(coff, nc, M.n_children_total) ? nc : 0;
            }
            if (c >= 0 && ((q != kCovis && M.kf_bad[c]) || kfpos[c] >= 0)) c = -1;
            s_cand[e] = c;
        }
        __syncthreads();
        if (wave == 0) {  // the walk itself on one wave, from LDS; the keyframes it appends are s_list[n_k1, n)
            int n = n_k1;
            bool bad = false;
            for (int it = 0; it < n_k1 && n <= kMaxKfs; ++it) {
                const int v = lane < kCandidates ? s_cand[it * kCandidates + lane] : -1;
                if (v == kBadId) bad = true;
                // the first of the best 10 covisibles that is not bad and not marked (:1691-1705)
                unsigned long long m = __ballot(lane < kCovis && v >= 0 && !appended(s_list, n_k1, n, v));
                if (m) {
                    const int add = __shfl(v, __ffsll((long long)m) - 1);
                    if (lane == 0) {
                        s_list[n] = add;
                        if (n < D.kf_stride) list[n] = add;
                    }
                    __builtin_amdgcn_wave_barrier();  // the other lanes read s_list[n] from here on
                    ++n;
                }
                // the first child that is not bad and not marked (:1708-1721); every child's id is checked
                bool found = false;
                m = __ballot(lane > kCovis && v >= 0 && !appended(s_list, n_k1, n, v));
                if (m) {
                    const int add = __shfl(v, __ffsll((long long)m) - 1);
                    if (lane == 0) {
                        s_list[n] = add;
                        if (n < D.kf_stride) list[n] = add;
                    }
                    __builtin_amdgcn_wave_barrier();
                    ++n;
                    found = true;
                }
                const int nc = s_nc[it];
                if (nc > kStagedChildren) {  // the rest of a long child list, from memory
                    const int coff = M.child_offset[s_list[it]];
                    for (int b = kStagedChildren; b < nc; b += 64) {
                        int ch = b + lane < nc ? M.children[coff + b + lane] : -1;
                        if (b + lane < nc && !in_range(ch, M.n_kf)) {
                            bad = true;
                            ch = -1;
                        }
                        const bool ok = ch >= 0 && !M.kf_bad[ch] && kfpos[ch] < 0;
                        m = __ballot(!found && ok && !appended(s_list, n_k1, n, ch));
                        if (m) {
                            const int add = __shfl(ch, __ffsll((long long)m) - 1);
                            if (lane == 0) {
                                s_list[n] = add;
                                if (n < D.kf_stride) list[n] = add;
                            }
                            __builtin_amdgcn_wave_barrier();
                            ++n;
                            found = true;
                        }
                    }
                }
                // the parent, bad or not; appending it ends the whole walk (:1724-1734)
                const int p = __shfl(v, kCovis);
                if (p >= 0 && !appended(s_list, n_k1, n, p)) {
                    if (lane == 0) {
                        s_list[n] = p;
                        if (n < D.kf_stride) list[n] = p;
                    }
                    ++n;
                    break;
                }
            }
            if (__ballot(bad) && lane == 0) s_bad = 1;
            if (lane == 0) s_n = n;
        }
    }
    __syncthreads();
    if (!kept && n_k1 > 0 && n_k1 <= kMaxKfs) n_list = s_n;
    int status = kPending;
    if (s_bad) status = ORBGPU_LOCALMAP_BAD_JOB;
    else if (n_list > D.kf_stride) status = kOverflow;
    // the slots before each list position: numbers every (position, slot) in UpdateLocalPoints' order
    if (status == kPending) {
        long long before = 0;
        bool bad = false;
        for (int s = 0; s < n_list; s += kThreads) {
            const int i = s + tid;
            long long c = 0;
            if (i < n_list) {
                const int kf = list[i];
                const int off = M.slot_offset[kf], ns = M.n_slots[kf];
                if (!span_ok(off, ns, M.n_slots_total)) bad = true;
                else c = ns;
            }
            long long incl = c;  // inclusive sum over the wave, then the waves before
            for (int d = 1; d < 64; d <<= 1) {
                const long long u = __shfl_up(incl, d);
                if (lane >= d) incl += u;
            }
            __syncthreads();
            if (lane == 63) s_red[wave] = incl;
            __syncthreads();
            long long pre = before, tot = 0;
            for (int w = 0; w < kThreads / 64; ++w) {
                if (w < wave) pre += s_red[w];
                tot += s_red[w];
            }
            if (i < n_list) V.kfbase[ol + i] = (int)min(pre + incl - c, 0x7fffffffLL);
            before += tot;
        }
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
        if (s_bad || before >= 0x7fffffffLL) status = ORBGPU_LOCALMAP_BAD_JOB;
    }
    if (tid == 0) {
        S.status = status;
        S.kept = kept;
        S.n_k1 = n_k1;
        S.n_list = n_list;
        S.ref_kf = (!kept && n_k1 > 0) ? (M.kf_by_rank ? M.kf_by_rank[0x7fffffff - (int)(unsigned)s_best]
                                                       : 0x7fffffff - (int)(unsigned)s_best)
                                       : -1;
    }
}

// ------------------------------------------------------------------ 4-6. the local points

__global__ __launch_bounds__(kThreads) void lm_mark_kernel(orbgpu_map_mirror M, Dims D, MWork V) {
    const int k = blockIdx.x, pos = blockIdx.y, tid = threadIdx.x;
    MState& S = V.st[k];
    if (S.status != kPending || pos >= S.n_list) return;
    const size_t opt = (size_t)k * (M.n_pt > 0 ? M.n_pt : 1), ol = (size_t)k * D.kf_stride;
    const int kf = V.list[ol + pos];
    const int off = M.slot_offset[kf], ns = M.n_slots[kf];
    const unsigned g0 = (unsigned)V.kfbase[ol + pos];
    bool bad = false;
    for (int s = tid; s < ns; s += kThreads) {
        const int id = M.slots[off + s];
        if (id == -1) continue;
        if (!in_range(id, M.n_pt)) bad = true;
        else if ((M.pt_flags[id] & ORBGPU_PT_VALID) && V.key[opt + id] > g0 + (unsigned)s)  // a stale read only costs an atomic
            atomicMin(&V.key[opt + id], g0 + (unsigned)s);
    }
    if (bad) S.bad_slot = 1;
}

// whether slot s of the keyframe at g0 is its point's first occurrence; id is checked
__device__ __forceinline__ bool first_seen(const orbgpu_map_mirror& M, const unsigned* key, int id, unsigned g) {
    return in_range(id, M.n_pt) && key[id] == g;
}

__global__ __launch_bounds__(kThreads) void lm_count_kernel(orbgpu_map_mirror M, Dims D, MWork V) {
    __shared__ long long s_red[kThreads / 64];
    const int k = blockIdx.x, pos = blockIdx.y, tid = threadIdx.x;
    const MState& S = V.st[k];
    if (S.status != kPending || S.bad_slot || pos >= S.n_list) return;
    const size_t opt = (size_t)k * (M.n_pt > 0 ? M.n_pt : 1), ol = (size_t)k * D.kf_stride;
    const int kf = V.list[ol + pos];
    const int off = M.slot_offset[kf], ns = M.n_slots[kf];
    const unsigned g0 = (unsigned)V.kfbase[ol + pos];
    int c = 0;
    for (int s = tid; s < ns; s += kThreads) c += first_seen(M, V.key + opt, M.slots[off + s], g0 + (unsigned)s);
    const long long t = block_sum(c, s_red);
    if (tid == 0) V.cnt[ol + pos] = (int)t;
}

// table entry idx of job J from the mirror's point id
__device__ __forceinline__ void gather_point(const orbgpu_update_local_map_job& J, const orbgpu_map_mirror& M, int idx,
                                             int id, int flags) {
    J.out_flags[idx] = flags;
    for (int c = 0; c < 3; ++c) {
        J.out_pos[3 * (size_t)idx + c] = M.pos[3 * (size_t)id + c];
        J.out_normal[3 * (size_t)idx + c] = M.normal[3 * (size_t)id + c];
    }
    const uint4* src = reinterpret_cast<const uint4*>(M.desc + 32 * (size_t)id);
    uint4* dst = reinterpret_cast<uint4*>(J.out_desc + 32 * (size_t)idx);
    dst[0] = src[0];
    dst[1] = src[1];
    J.out_min_dist[idx] = M.min_dist[id];
    J.out_max_dist[idx] = M.max_dist[id];
}

__global__ __launch_bounds__(kThreads) void lm_scatter_kernel(const orbgpu_update_local_map_job* __restrict__ jobs,
                                                              orbgpu_map_mirror M, Dims D, MWork V,
                                                              int* __restrict__ local_points) {
    __shared__ long long s_red[kThreads / 64];
    __shared__ int s_wave[kThreads / 64];
    const int k = blockIdx.x, pos = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MState& S = V.st[k];
    if (S.status != kPending || S.bad_slot || pos >= S.n_list) return;
    const size_t opt = (size_t)k * (M.n_pt > 0 ? M.n_pt : 1), ol = (size_t)k * D.kf_stride;
    if (V.cnt[ol + pos] == 0) return;
    const orbgpu_update_local_map_job& J = jobs[k];
    long long before = 0;  // the first occurrences in the keyframes before this one
    for (int i = tid; i < pos; i += kThreads) before += V.cnt[ol + i];
    before = block_sum(before, s_red);
    const int kf = V.list[ol + pos];
    const int off = M.slot_offset[kf], ns = M.n_slots[kf];
    const unsigned g0 = (unsigned)V.kfbase[ol + pos];
    int* lp = local_points + (size_t)k * D.point_stride;
    int base = 0;
    for (int s0 = 0; s0 < ns; s0 += kThreads) {
        const int s = s0 + tid;
        const int id = s < ns ? M.slots[off + s] : -1;
        const bool ok = s < ns && first_seen(M, V.key + opt, id, g0 + (unsigned)s);
        const int r = compact_slot(ok, lane, wave, s_wave, base);
        if (ok) {
            const long long idx = before + r;
            V.tix[opt + id] = (int)min(idx, 0x7fffffffLL);
            if (idx < D.point_stride) {
                lp[idx] = id;
                const unsigned pm = V.pm[opt + id];
                const int seen = (pm & kInRow0) && !(pm & kInRow1) ? ORBGPU_PT_LAST_SEEN : 0;  // culled by call 1
                gather_point(J, M, (int)idx, id, ORBGPU_PT_VALID | (M.pt_flags[id] & ORBGPU_PT_HAS_OBS) | seen);
            }
        }
        compact_advance<kThreads>(s_wave, base);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ 7. the frame's side

__global__ __launch_bounds__(kThreads) void lm_finish_kernel(const orbgpu_update_local_map_job* __restrict__ jobs,
                                                             orbgpu_map_mirror M, Dims D, MWork V,
                                                             orbgpu_update_local_map_result* __restrict__ results,
                                                             int* __restrict__ local_kfs) {
    __shared__ long long s_red[kThreads / 64];
    __shared__ int s_wave[kThreads / 64];
    __shared__ int s_kp[kMaxKps];   // the keypoints that hold a point outside the local map, ascending
    __shared__ int s_id[kMaxKps];   // that point: the mirror id, or ~t for entry t of call 1's table
    __shared__ int s_own[kMaxKps];  // the first list entry with the same point; then -1 - its rank
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MState& S = V.st[k];
    const orbgpu_update_local_map_job& J = jobs[k];
    orbgpu_update_local_map_result& R = results[k];
    int status = S.status;
    if (status == kPending && S.bad_slot) status = ORBGPU_LOCALMAP_BAD_JOB;
    if (status == ORBGPU_LOCALMAP_BAD_JOB) {
        if (tid == 0) {
            R.status = ORBGPU_LOCALMAP_BAD_JOB;
            R.n_k1 = R.n_local_kfs = R.n_nulled = R.n_local = R.n_extra = R.pad = 0;
            R.ref_kf = -1;
            if (J.local_job) J.local_job->frame = -1;  // call 2 reports ORBGPU_TRACK_BAD_JOB
        }
        return;
    }
    const size_t opt = (size_t)k * (M.n_pt > 0 ? M.n_pt : 1), ol = (size_t)k * D.kf_stride;
    const int n_list = S.n_list;
    for (int i = tid; i < min(n_list, D.kf_stride); i += kThreads) local_kfs[ol + i] = V.list[ol + i];
    if (status == kOverflow) {  // the keypoints or the keyframes do not fit: no point was gathered
        for (int j = tid; j < D.stride; j += kThreads) J.frame_mp[j] = -1;
        if (tid == 0) {
            R.status = ORBGPU_LOCALMAP_CAPACITY;
            R.n_k1 = S.n_k1;
            R.n_local_kfs = n_list;
            R.ref_kf = S.ref_kf;
            R.n_nulled = S.n_nulled;
            R.n_local = R.n_extra = R.pad = 0;
        }
    }
    int n_local = 0, n_extra = 0;
    if (status == kPending) {
        long long sum = 0;
        for (int i = tid; i < n_list; i += kThreads) sum += V.cnt[ol + i];
        n_local = (int)min(block_sum(sum, s_red), 0x7fffffffLL);
        // mvpMapPoints after :1627-1644: a local point's table index, NULL, or an extra
        const int* row1 = J.rows + D.stride;
        int n_cand = 0;
        for (int s = 0; s < J.n_kp; s += kThreads) {
            const int j = s + tid;
            int mp = -1, id = -1;
            bool extra = false;
            if (j < J.n_kp) {
                const int t = row1[j];
                if (t >= 0) {  // t < src_n and the id's range were checked by lm_vote_kernel
                    id = J.src_pt_id[t];
                    if (id < 0) {
                        extra = true;
                        id = ~t;
                    } else if (M.pt_flags[id] & ORBGPU_PT_VALID) {
                        if (V.key[opt + id] != kNoKey) mp = V.tix[opt + id];
                        else extra = true;
                    }
                }
                if (!extra) J.frame_mp[j] = mp;
            }
            const int m = compact_slot(extra, lane, wave, s_wave, n_cand);
            if (extra) {
                s_kp[m] = j;
                s_id[m] = id;
            }
            compact_advance<kThreads>(s_wave, n_cand);
            __syncthreads();
        }
        for (int j = J.n_kp + tid; j < D.stride; j += kThreads) J.frame_mp[j] = -1;
        for (int m = tid; m < n_cand; m += kThreads) {  // a point held at two keypoints is one extra
            const int id = s_id[m];
            int own = m;
            for (int a = 0; a < m; ++a)
                if (s_id[a] == id) {
                    own = a;
                    break;
                }
            s_own[m] = own;
        }
        __syncthreads();
        for (int s = 0; s < n_cand; s += kThreads) {  // the owners' ranks, in keypoint order
            const int m = s + tid;
            const bool first = m < n_cand && s_own[m] == m;
            const int r = compact_slot(first, lane, wave, s_wave, n_extra);
            if (first) s_own[m] = -1 - r;
            compact_advance<kThreads>(s_wave, n_extra);
            __syncthreads();
        }
        for (int m = tid; m < n_cand; m += kThreads) {
            const int o = s_own[m];
            const bool first = o < 0;
            const long long idx = (long long)n_local + (first ? -1 - o : -1 - s_own[o]);
            J.frame_mp[s_kp[m]] = (int)min(idx, 0x7fffffffLL);
            if (!first || idx >= D.point_stride) continue;
            const int id = s_id[m];
            if (id >= 0) {  // a map point outside the local map
                gather_point(J, M, (int)idx, id, ORBGPU_PT_VALID | (M.pt_flags[id] & ORBGPU_PT_HAS_OBS));
            } else {  // a temporal point: call 1's entry; SearchLocalPoints projects no held point
                const int t = ~id;
                J.out_flags[idx] = ORBGPU_PT_VALID;
                for (int c = 0; c < 3; ++c) {
                    J.out_pos[3 * (size_t)idx + c] = J.src_pos[3 * (size_t)t + c];
                    J.out_normal[3 * (size_t)idx + c] = 0.f;
                }
                const uint4* src = reinterpret_cast<const uint4*>(J.src_desc + 32 * (size_t)t);
                uint4* dst = reinterpret_cast<uint4*>(J.out_desc + 32 * (size_t)idx);
                dst[0] = src[0];
                dst[1] = src[1];
                J.out_min_dist[idx] = 0.f;
                J.out_max_dist[idx] = 0.f;
            }
        }
    }
    if (tid == 0) {
        const long long total = (long long)n_local + n_extra;
        if (status == kPending) {
            R.status = total > D.point_stride ? ORBGPU_LOCALMAP_CAPACITY
                                              : (S.kept ? ORBGPU_LOCALMAP_KEPT : ORBGPU_LOCALMAP_OK);
            R.n_k1 = S.n_k1;
            R.n_local_kfs = n_list;
            R.ref_kf = S.ref_kf;
            R.n_nulled = S.n_nulled;
            R.n_local = n_local;
            R.n_extra = n_extra;
            R.pad = 0;
        }
        orbgpu_track_local_job& L = *J.local_job;
        L.n_local = n_local;
        L.points.n = status == kOverflow ? D.point_stride + 1 : (int)min(total, 0x7fffffffLL);
        L.points.flags = J.out_flags;
        L.points.pos = J.out_pos;
        L.points.normal = J.out_normal;
        L.points.desc = J.out_desc;
        L.points.min_dist = J.out_min_dist;
        L.points.max_dist = J.out_max_dist;
        L.frame_mp = J.frame_mp;
    }
}

bool fits_int(long long a, long long b) { return a * b <= 0x7fffffffLL; }

const char* mirror_error(const orbgpu_map_mirror* m) {
    if (!m) return "mirror is NULL";
    if (m->n_kf < 0 || m->n_pt < 0 || m->n_slots_total < 0 || m->n_children_total < 0 || m->n_obs_total < 0)
        return "a mirror count is negative";
    if (m->n_kf > 0 && (!m->kf_bad || !m->slot_offset || !m->n_slots || !m->covis || !m->child_offset ||
                        !m->n_children || !m->parent))
        return "a keyframe array of the mirror is NULL";
    if (m->n_pt > 0 && (!m->pt_flags || !m->obs_offset || !m->n_obs || !m->pos || !m->normal || !m->desc ||
                        !m->min_dist || !m->max_dist))
        return "a point array of the mirror is NULL";
    if ((m->n_slots_total > 0 && !m->slots) || (m->n_children_total > 0 && !m->children) ||
        (m->n_obs_total > 0 && !m->obs))
        return "slots, children or obs is NULL";
    return nullptr;
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

size_t orbgpu_update_local_map_workspace_bytes(int n, int stride, int point_stride, int kf_stride, int n_kf,
                                               int n_pt) {
    const long long N = n > 0 ? n : 1;
    (void)stride;
    (void)point_stride;
    if (!fits_int(N, kf_stride > 0 ? kf_stride : 1)) return 0;
    size_t bytes = 0;
    carve(nullptr, n, kf_stride, n_kf, n_pt, &bytes);
    return bytes;
}

int orbgpu_update_local_map_batch_device(int n, const orbgpu_update_local_map_job* d_jobs,
                                         const orbgpu_map_mirror* mirror, int stride, int point_stride,
                                         int kf_stride, void* d_workspace,
                                         orbgpu_update_local_map_result* d_results, int* d_local_kfs,
                                         int* d_local_points, void* stream) {
    if (n < 0 || stride <= 0 || point_stride <= 0 || kf_stride <= 0 ||
        (n > 0 && (!d_jobs || !d_workspace || !d_results || !d_local_kfs || !d_local_points)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if (kf_stride > 65535) return fail(ORBGPU_ERR_ARG, "kf_stride above 65535");
    if (n > 0 || mirror)
        if (const char* e = mirror_error(mirror)) return fail(ORBGPU_ERR_ARG, e);
    if (!fits_int(n, 2LL * stride) || !fits_int(n, point_stride) || !fits_int(n, kf_stride))
        return fail(ORBGPU_ERR_ARG, "n * stride, n * point_stride or n * kf_stride overflows");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const orbgpu_map_mirror M = *mirror;
    const Dims D{stride, point_stride, kf_stride};
    const MWork V = carve(d_workspace, n, kf_stride, M.n_kf, M.n_pt, nullptr);
    const dim3 block(kThreads), per_job(n), per_kf(n, kf_stride);
    const int most = M.n_pt > M.n_kf ? (M.n_pt > kf_stride ? M.n_pt : kf_stride) : (M.n_kf > kf_stride ? M.n_kf : kf_stride);
    const int chunks = (most + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(lm_clear_kernel, dim3(n, chunks < 1024 ? chunks : 1024), block, 0, s, V, M.n_kf, M.n_pt, kf_stride);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_vote_kernel, per_job, dim3(kVoteThreads), 0, s, d_jobs, M, D, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_walk_kernel, per_job, block, 0, s, d_jobs, M, D, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_mark_kernel, per_kf, block, 0, s, M, D, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_count_kernel, per_kf, block, 0, s, M, D, V);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_scatter_kernel, per_kf, block, 0, s, d_jobs, M, D, V, d_local_points);
    ORB_HIP(hipGetLastError());
    hipLaunchKernelGGL(lm_finish_kernel, per_job, block, 0, s, d_jobs, M, D, V, d_results, d_local_kfs);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

}  // extern "C"
