// covis.hip -- the covisibility graph as a table in HBM (include/orbgpu_covis.h) and the covisibility
// part of KeyFrame::SetBadFlag on it (src/KeyFrame.cpp:572-573, :584-585, with EraseConnection :677-691
// and UpdateBestCovisibles :161-184).
//
//  orbgpu_covis_erase_keyframes_batch_device: one launch, erase_kernel.  A single workgroup walks the
//  listed keyframes in order; its sixteen waves take the entries of the erased keyframe's conn row, one
//  neighbour each: the wave finds the key in the neighbour's row, moves the entries behind it one place
//  down, and rebuilds the neighbour's ordered row by ranking the unique keys (weight, position in the row).
//  Then the erased keyframe's own rows are cleared.
//
//  orbgpu_covis_update_connections_batch_device: KeyFrame::UpdateConnections (:369-483, AddConnection :140-154).
//  update_clear_kernel and update_rank_kernel prepare the workspace (the inverse of kf_by_rank, zeroed counters),
//  update_count_kernel takes KFcounter of every job in parallel with integer atomics, and update_apply_kernel, a
//  single workgroup, applies the jobs in list order: two walks over the counters in rank order (sizes and the
//  first strict maximum; the compaction into LDS), a wave per member of the ordered set that first asks whether
//  its neighbour has room and then inserts or overwrites the key and rebuilds that neighbour's ordered row, and
//  the keyframe's own rows from LDS.
//
//  orbgpu_covis_keyframe_culling_batch_device: the judging loop of LocalMapping::KeyFrameCulling
//  (src/LocalMapping.cpp:802-880), cull_kernel, a workgroup per job.  It walks the job's list in order, its
//  threads over the slots of the judged keyframe; the keyframes it has culled are a hash set in LDS, through
//  which a later verdict sees SetBadFlag's erased observations (MapPoint.cpp:141-169).  It writes neither the
//  table nor the mirrors.
//
// Positions come from ranks over unique keys, so every output byte is a function of the list and the
// table.  Nothing synchronises with the host or with another workgroup.  Every count and id read from the
// list or the table is range-checked before it is used as an index.  The steps of the walk are ordered by
// __syncthreads() (a workgroup-scope release and acquire); the table, which the launch writes too, is
// read through agent-scope relaxed loads, which are never moved to the scalar cache.
#include "../../include/orbgpu_covis.h"
#include "host_common.h"

namespace orbgpu {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

static_assert(ORBGPU_COVIS_BEST == ORBGPU_LOCALMAP_COVIS, "covis10 is the first mirror's covis");

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

// a word of the table, which this launch writes too
__device__ __forceinline__ int tld(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (weight, position) as one unsigned key in the order of std::pair<int, KeyFrame*>
__device__ __forceinline__ unsigned long long order_key(int w, int pos) {
    return ((unsigned long long)((unsigned)w ^ 0x80000000u) << 32) | (unsigned)pos;
}

// ---- a row of the table, one wave

// the first position of `key` among the n entries of keyframe nb's conn row, -1: absent
__device__ __forceinline__ int find_key(const orbgpu_covis_graph& G, int nb, int n, int key, int lane) {
    const size_t row = (size_t)nb * G.conn_stride;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const unsigned long long m = __ballot(i < n && tld(G.conn_kf + row + i) == key);
        if (m) return c0 + (int)__ffsll((long long)m) - 1;
    }
    return -1;
}

// UpdateBestCovisibles (:161-184) of keyframe nb from its conn row of n entries
__device__ __forceinline__ void rebuild_ordered(const orbgpu_covis_graph& G, int nb, int n, int lane) {
    const size_t row = (size_t)nb * G.conn_stride;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const int kfi = i < n ? tld(G.conn_kf + row + i) : -1, wi = i < n ? tld(G.conn_w + row + i) : 0;
        const unsigned long long ki = order_key(wi, i);
        int r = 0;  // the entries that sort before this one: descending (weight, position)
        for (int d0 = 0; d0 < n; d0 += 64) {
            const int j = d0 + lane;
            const unsigned long long kj = j < n ? order_key(tld(G.conn_w + row + j), j) : 0ull;
            const int m = n - d0 < 64 ? n - d0 : 64;
            for (int t = 0; t < m; ++t) r += __shfl(kj, t) > ki;
        }
        if (i < n) {  // unique keys: r < n
            G.ord_kf[row + r] = kfi;
            G.ord_w[row + r] = wi;
            if (r < ORBGPU_COVIS_BEST) G.covis10[(size_t)nb * ORBGPU_COVIS_BEST + r] = kfi;
        }
    }
    if (lane < ORBGPU_COVIS_BEST && lane >= n) G.covis10[(size_t)nb * ORBGPU_COVIS_BEST + lane] = -1;
    if (lane == 0) G.n_ord[nb] = n;
}

// nb->EraseConnection(key) (:677-691)
__device__ __forceinline__ void erase_connection(const orbgpu_covis_graph& G, int nb, int key, int lane) {
    const size_t row = (size_t)nb * G.conn_stride;
    const int n = tld(G.n_conn + nb);
    if (n <= 0 || n > G.conn_stride) return;
    const int found = find_key(G, nb, n, key, lane);
    if (found < 0) return;  // :682
    // (found, n) one place down, from the bottom: a chunk reads nothing an earlier chunk wrote
    for (int lo = found; lo < n - 1; lo += 64) {
        const int i = lo + lane;
        const bool act = i < n - 1;
        const int a = act ? tld(G.conn_kf + row + i + 1) : 0, b = act ? tld(G.conn_w + row + i + 1) : 0;
        if (act) {
            G.conn_kf[row + i] = a;
            G.conn_w[row + i] = b;
        }
    }
    if (lane == 0) G.n_conn[nb] = n - 1;
    __threadfence_block();  // the row as this wave's other lanes wrote it
    rebuild_ordered(G, nb, n - 1, lane);
}

__global__ __launch_bounds__(kThreads) void erase_kernel(int n, const int* __restrict__ kfs, orbgpu_covis_graph G, int* status) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = G.conn_stride;
    for (int e = 0; e < n; ++e) {
        const int x = kfs[e];
        if (!in_range(x, G.n_kf)) {  // uniform
            if (tid == 0) status[e] = ORBGPU_COVIS_BAD_JOB;
            continue;
        }
        const size_t row = (size_t)x * stride;
        int nx = tld(G.n_conn + x);
        nx = nx < 0 ? 0 : nx > stride ? stride : nx;
        // the entries of x's row are distinct and none is x: every wave has a row of its own
        for (int j = wave; j < nx; j += kWaves) {  // :572-573
            const int nb = tld(G.conn_kf + row + j);
            if (in_range(nb, G.n_kf) && nb != x) erase_connection(G, nb, x, lane);
        }
        __syncthreads();
        if (tid < ORBGPU_COVIS_BEST) G.covis10[(size_t)x * ORBGPU_COVIS_BEST + tid] = -1;
        if (tid == 0) {  // :584-585
            G.n_conn[x] = 0;
            G.n_ord[x] = 0;
            status[e] = ORBGPU_COVIS_OK;
        }
        __syncthreads();  // the next keyframe reads these rows
    }
}

// ---- UpdateConnections ---------------------------------------------------------------------------------

constexpr int kCountThreads = 256;
constexpr int kCountChunks = 4;  // workgroups over the slots of one job's keyframe

// the workspace: rank_of[n_kf], the inverse of kf_by_rank; flags[0]: a kf_by_rank entry outside the mirror,
// flags[1 + j]: job j read an index outside the mirror; counts[j * n_kf + k]: KFcounter of job j
struct UpdateWs {
    int* rank_of;
    int* flags;
    int* counts;
};

inline long long update_ws_ints(int n, int n_kf) { return (long long)n_kf + 1 + n + (long long)n * n_kf; }

inline UpdateWs update_ws(void* p, int n, int n_kf) {
    int* w = static_cast<int*>(p);
    return {w, w + n_kf, w + n_kf + 1 + n};
}

__device__ __forceinline__ bool range_ok(int off, int cnt, int total) {
    return off >= 0 && cnt >= 0 && (long long)off + cnt <= (long long)total;
}

// rank_of = the identity (kf_by_rank NULL), the flags and the counts zero
__global__ __launch_bounds__(kCountThreads) void update_clear_kernel(int* ws, int n_kf, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        ws[i] = i < n_kf ? (int)i : 0;
}

__global__ __launch_bounds__(kCountThreads) void update_rank_kernel(const int* __restrict__ by_rank, int n_kf, UpdateWs W) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_kf; r += gridDim.x * blockDim.x) {
        const int k = by_rank[r];
        if (in_range(k, n_kf))
            W.rank_of[k] = r;
        else
            W.flags[0] = 1;
    }
}

// KFcounter (:388-408) of job blockIdx.x; blockIdx.y: a share of the keyframe's slots
__global__ __launch_bounds__(kCountThreads) void update_count_kernel(const int* __restrict__ kfs, orbgpu_map_mirror M, UpdateWs W) {
    const int job = blockIdx.x, x = kfs[job];
    bool bad = !in_range(x, M.n_kf);
    if (!bad) {
        const int off = M.slot_offset[x], ns = M.n_slots[x];
        bad = !range_ok(off, ns, M.n_slots_total);
        int* cnt = W.counts + (size_t)job * M.n_kf;
        for (int s = blockIdx.y * blockDim.x + threadIdx.x; !bad && s < ns; s += gridDim.y * blockDim.x) {
            const int p = M.slots[off + s];
            if (p == -1) continue;  // :392
            if (!in_range(p, M.n_pt)) {
                bad = true;
                break;
            }
            if (!(M.pt_flags[p] & ORBGPU_PT_VALID)) continue;  // :395
            const int oo = M.obs_offset[p], no = M.n_obs[p];
            if (!range_ok(oo, no, M.n_obs_total)) {
                bad = true;
                break;
            }
            for (int i = 0; i < no; ++i) {
                const int k = M.obs[oo + i];
                if (!in_range(k, M.n_kf))
                    bad = true;
                else if (k != x)  // :404
                    atomicAdd(cnt + k, 1);
            }
        }
    }
    if (bad) W.flags[1 + job] = 1;
}

// nb->AddConnection(key, w) (:140-154); nb's count lies in [0, conn_stride], below it when the key is absent
__device__ __forceinline__ void add_connection(const orbgpu_covis_graph& G, const int* rank_of, int nb, int key, int w, int lane) {
    const size_t row = (size_t)nb * G.conn_stride;
    const int n = tld(G.n_conn + nb);
    const int found = find_key(G, nb, n, key, lane);
    if (found >= 0) {
        if (tld(G.conn_w + row + found) == w) return;  // :149-150
        if (lane == 0) G.conn_w[row + found] = w;
        __threadfence_block();
        rebuild_ordered(G, nb, n, lane);
        return;
    }
    // the key's place in the row: behind the entries of lower rank
    const int rk = rank_of[key];
    int p = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        bool lower = false;
        if (i < n) {
            const int k = tld(G.conn_kf + row + i);
            lower = in_range(k, G.n_kf) && rank_of[k] < rk;
        }
        p += __popcll(__ballot(lower));
    }
    // [p, n) one place up, from the top: a chunk reads nothing an earlier chunk wrote
    for (int hi = n; hi > p; hi -= 64) {
        const int i = hi - 1 - lane;
        const bool act = i >= p;
        const int a = act ? tld(G.conn_kf + row + i) : 0, b = act ? tld(G.conn_w + row + i) : 0;
        if (act) {
            G.conn_kf[row + i + 1] = a;
            G.conn_w[row + i + 1] = b;
        }
    }
    if (lane == 0) {
        G.conn_kf[row + p] = key;
        G.conn_w[row + p] = w;
        G.n_conn[nb] = n + 1;
    }
    __threadfence_block();
    rebuild_ordered(G, nb, n + 1, lane);
}

__device__ __forceinline__ void update_result(orbgpu_covis_update_result* r, int status, int n_counted, int n_ordered, int kf_max,
                                              int w_max) {
    r->status = status;
    r->n_counted = n_counted;
    r->n_ordered = n_ordered;
    r->kf_max = kf_max;
    r->w_max = w_max;
    r->front = -1;
    r->pad[0] = r->pad[1] = 0;
}

// one workgroup applies the jobs in list order (:417-471)
__global__ __launch_bounds__(kThreads) void update_apply_kernel(int n, const int* __restrict__ kfs, const int* __restrict__ by_rank,
                                                                orbgpu_covis_graph G, UpdateWs W, orbgpu_covis_update_result* results) {
    __shared__ int s_kf[ORBGPU_COVIS_MAX_STRIDE], s_w[ORBGPU_COVIS_MAX_STRIDE];  // KFcounter in rank order
    __shared__ int s_a[kWaves], s_b[kWaves];
    __shared__ unsigned long long s_best[kWaves];
    __shared__ int s_imax, s_cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_kf = G.n_kf, stride = G.conn_stride;
    const bool rank_bad = W.flags[0] != 0;
    for (int e = 0; e < n; ++e) {
        const int x = kfs[e];
        if (rank_bad || W.flags[1 + e] || !in_range(x, n_kf)) {  // uniform
            if (tid == 0) update_result(results + e, ORBGPU_COVIS_BAD_JOB, 0, 0, -1, 0);
            continue;
        }
        const int* cnt = W.counts + (size_t)e * n_kf;
        // the size of the counter, the members with w >= th and the first strict maximum in rank order
        int n_counted = 0, n_th = 0;
        unsigned long long best = 0;
        for (int r = tid; r < n_kf; r += kThreads) {
            const int c = cnt[by_rank ? by_rank[r] : r];
            if (c > 0) {
                ++n_counted;
                n_th += c >= ORBGPU_COVIS_TH;
                const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7fffffff - r);
                best = key > best ? key : best;
            }
        }
        for (int o = 32; o; o >>= 1) {
            n_counted += __shfl_xor(n_counted, o);
            n_th += __shfl_xor(n_th, o);
            const unsigned long long b = __shfl_xor(best, o);
            best = b > best ? b : best;
        }
        if (lane == 0) {
            s_a[wave] = n_counted;
            s_b[wave] = n_th;
            s_best[wave] = best;
        }
        if (tid == 0) s_cap = 0;
        __syncthreads();
        n_counted = n_th = 0;
        best = 0;
        for (int v = 0; v < kWaves; ++v) {
            n_counted += s_a[v];
            n_th += s_b[v];
            best = s_best[v] > best ? s_best[v] : best;
        }
        __syncthreads();  // s_a is used again below
        if (n_counted == 0) {  // :411
            if (tid == 0) update_result(results + e, ORBGPU_COVIS_EMPTY, 0, 0, -1, 0);
            continue;
        }
        const int r_max = 0x7fffffff - (int)(unsigned)(best & 0xffffffffu), w_max = (int)(best >> 32);
        const int kf_max = by_rank ? by_rank[r_max] : r_max;
        const int n_ordered = n_th > 0 ? n_th : 1;  // :444-451
        if (n_counted > stride) {
            if (tid == 0) update_result(results + e, ORBGPU_COVIS_CAPACITY, n_counted, n_ordered, kf_max, w_max);
            continue;
        }
        // the counter into LDS in rank order
        for (int r0 = 0, base = 0; r0 < n_kf; r0 += kThreads) {
            const int r = r0 + tid;
            const int k = r < n_kf ? (by_rank ? by_rank[r] : r) : 0, c = r < n_kf ? cnt[k] : 0;
            const unsigned long long m = __ballot(c > 0);
            if (lane == 0) s_a[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
            for (int v = 0; v < kWaves; ++v) {
                before += v < wave ? s_a[v] : 0;
                total += s_a[v];
            }
            if (c > 0) {
                const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));  // < n_counted <= stride
                s_kf[pos] = k;
                s_w[pos] = c;
                if (r == r_max) s_imax = pos;
            }
            base += total;
            __syncthreads();
        }
        const int i_max = s_imax;
        // the members of the ordered set: a wave each, their rows are distinct.  First: is there room?
        for (int i = wave; i < n_counted; i += kWaves) {
            if (!(n_th > 0 ? s_w[i] >= ORBGPU_COVIS_TH : i == i_max)) continue;
            const int nb = s_kf[i], m = tld(G.n_conn + nb);
            if (m < 0 || m > stride || (m == stride && find_key(G, nb, m, x, lane) < 0)) s_cap = 1;
        }
        __syncthreads();
        const bool cap = s_cap != 0;
        __syncthreads();  // s_cap is cleared by the next job
        if (cap) {
            if (tid == 0) update_result(results + e, ORBGPU_COVIS_CAPACITY, n_counted, n_ordered, kf_max, w_max);
            continue;
        }
        if (tid == 0) update_result(results + e, ORBGPU_COVIS_OK, n_counted, n_ordered, kf_max, w_max);  // front: below
        for (int i = wave; i < n_counted; i += kWaves)  // :439, :450
            if (n_th > 0 ? s_w[i] >= ORBGPU_COVIS_TH : i == i_max) add_connection(G, W.rank_of, s_kf[i], x, s_w[i], lane);
        __syncthreads();
        // the keyframe's own rows (:469-471): n_counted <= kThreads
        const size_t row = (size_t)x * stride;
        if (tid < n_counted) {
            G.conn_kf[row + tid] = s_kf[tid];
            G.conn_w[row + tid] = s_w[tid];
            if (n_th > 0 ? s_w[tid] >= ORBGPU_COVIS_TH : tid == i_max) {
                const unsigned long long ki = order_key(s_w[tid], tid);
                int r = 0;  // the members that sort before this one: descending (weight, position)
                if (n_th > 0)
                    for (int j = 0; j < n_counted; ++j) r += s_w[j] >= ORBGPU_COVIS_TH && order_key(s_w[j], j) > ki;
                G.ord_kf[row + r] = s_kf[tid];
                G.ord_w[row + r] = s_w[tid];
                if (r < ORBGPU_COVIS_BEST) G.covis10[(size_t)x * ORBGPU_COVIS_BEST + r] = s_kf[tid];
                if (r == 0) results[e].front = s_kf[tid];  // after the barrier that follows thread 0's -1
            }
        }
        if (tid < ORBGPU_COVIS_BEST && tid >= n_ordered) G.covis10[(size_t)x * ORBGPU_COVIS_BEST + tid] = -1;
        if (tid == 0) {
            G.n_conn[x] = n_counted;
            G.n_ord[x] = n_ordered;
        }
        __syncthreads();  // the next job reads these rows
    }
}

// ---- KeyFrameCulling ----------------------------------------------------------------------------------

constexpr int kCullHash = 2 * ORBGPU_COVIS_MAX_STRIDE;  // the culled set: open addressing, at most half full

__device__ __forceinline__ unsigned cull_hash(int k) { return ((unsigned)k * 2654435761u) >> 21; }
static_assert(kCullHash == 1 << 11, "cull_hash gives 11 bits");

__device__ __forceinline__ bool culled_has(const int* tab, int k) {
    for (unsigned h = cull_hash(k);; h = (h + 1) & (kCullHash - 1)) {
        const int v = tab[h];
        if (v == k) return true;
        if (v < 0) return false;
    }
}

__global__ __launch_bounds__(kThreads) void cull_kernel(const orbgpu_covis_cull_job* __restrict__ jobs, orbgpu_map_mirror M,
                                                        orbgpu_map_mirror_ba B, orbgpu_map_mirror_cull C, orbgpu_covis_graph G,
                                                        int list_stride, orbgpu_covis_cull_result* results,
                                                        orbgpu_covis_cull_verdict* verdicts, int* culled) {
    __shared__ int s_list[ORBGPU_COVIS_MAX_STRIDE], s_verdict[ORBGPU_COVIS_MAX_STRIDE];
    __shared__ int s_mps[ORBGPU_COVIS_MAX_STRIDE], s_red[ORBGPU_COVIS_MAX_STRIDE];
    __shared__ int s_tab[kCullHash];
    __shared__ int s_cnt[3];  // nMPs, nRedundantObservations, an index outside the mirror
    const int tid = threadIdx.x, lane = tid & 63, job = blockIdx.x;
    const int kf = jobs[job].kf;
    const bool mono = jobs[job].mono != 0;
    int* crow = culled + (size_t)job * list_stride;
    orbgpu_covis_cull_verdict* vrow = verdicts + (size_t)job * list_stride;
    int status = ORBGPU_COVIS_OK, n_list = 0, n_culled = 0, n_tbe = 0;
    if (!in_range(kf, G.n_kf)) {
        status = ORBGPU_COVIS_BAD_JOB;
    } else {
        n_list = G.n_ord[kf];
        if (n_list < 0 || n_list > G.conn_stride) {
            status = ORBGPU_COVIS_BAD_JOB;
            n_list = 0;
        } else if (n_list > list_stride) {
            status = ORBGPU_COVIS_CAPACITY;
        }
    }
    if (status == ORBGPU_COVIS_OK) {  // uniform
        for (int i = tid; i < n_list; i += kThreads) s_list[i] = G.ord_kf[(size_t)kf * G.conn_stride + i];  // the snapshot, :810
        for (int i = tid; i < kCullHash; i += kThreads) s_tab[i] = -1;
        if (tid == 0) s_cnt[2] = 0;
        __syncthreads();
        bool bad = false;
        for (int e = 0; e < n_list && !bad; ++e) {
            const int k = s_list[e];
            if (tid == 0) s_cnt[0] = s_cnt[1] = 0;
            __syncthreads();
            if (!in_range(k, M.n_kf)) {
                bad = true;
                break;
            }
            int verdict = ORBGPU_COVIS_CULL_SKIPPED_FIRST, n_mps = 0, n_red = 0;
            if (!B.kf_first[k]) {  // :816
                const int off = M.slot_offset[k], ns = M.n_slots[k];
                if (!range_ok(off, ns, M.n_slots_total)) {
                    bad = true;
                    break;
                }
                const float th_depth = C.kf_th_depth[k];
                int my_mps = 0, my_red = 0;
                bool my_bad = false;
                for (int s = tid; s < ns; s += kThreads) {
                    const int p = M.slots[off + s];
                    if (p == -1) continue;  // :830
                    if (!in_range(p, M.n_pt)) {
                        my_bad = true;
                        continue;
                    }
                    if (!(M.pt_flags[p] & ORBGPU_PT_VALID)) continue;  // :832
                    const int oo = M.obs_offset[p], no = M.n_obs[p];
                    if (!range_ok(oo, no, M.n_obs_total)) {
                        my_bad = true;
                        continue;
                    }
                    // Observations() without the culled observers, and whether one of them was culled
                    int n_obs = 0;
                    bool lost = false, p_bad = false;
                    for (int i = 0; i < no; ++i) {
                        const int o = M.obs[oo + i], oi = B.obs_idx[oo + i];
                        if (!in_range(o, M.n_kf)) {
                            p_bad = true;
                            break;
                        }
                        const int so = M.slot_offset[o], sn = M.n_slots[o];
                        if (!range_ok(so, sn, M.n_slots_total) || !in_range(oi, sn)) {
                            p_bad = true;
                            break;
                        }
                        if (n_culled && culled_has(s_tab, o))
                            lost = true;
                        else
                            n_obs += B.kp_obs[(size_t)(so + oi) * 3 + 2] >= 0.0f ? 2 : 1;
                    }
                    if (p_bad) {
                        my_bad = true;
                        continue;
                    }
                    if (lost && n_obs <= 2) continue;  // MapPoint.cpp:162: bad since an earlier verdict
                    if (!mono) {
                        const float d = C.kp_depth[off + s];
                        if (d > th_depth || d < 0.0f) continue;  // :837
                    }
                    ++my_mps;
                    if (n_obs > 3) {  // :843
                        const int level = C.kp_octave[off + s];
                        int seen = 0;
                        for (int i = 0; i < no && seen < 3; ++i) {
                            const int o = M.obs[oo + i];
                            if (o == k || (n_culled && culled_has(s_tab, o))) continue;
                            seen += (int)C.kp_octave[M.slot_offset[o] + B.obs_idx[oo + i]] <= level + 1;  // :858
                        }
                        my_red += seen >= 3;
                    }
                }
                for (int o = 32; o; o >>= 1) {
                    my_mps += __shfl_xor(my_mps, o);
                    my_red += __shfl_xor(my_red, o);
                }
                if (lane == 0 && my_mps) atomicAdd(&s_cnt[0], my_mps);
                if (lane == 0 && my_red) atomicAdd(&s_cnt[1], my_red);
                if (my_bad) s_cnt[2] = 1;
                __syncthreads();
                n_mps = s_cnt[0];
                n_red = s_cnt[1];
                if (s_cnt[2]) {
                    bad = true;
                    break;
                }
                const bool redundant = (double)n_red > 0.9 * (double)n_mps;  // :877
                verdict = !redundant ? ORBGPU_COVIS_CULL_KEPT
                          : C.kf_not_erase[k] ? ORBGPU_COVIS_CULL_TO_BE_ERASED  // KeyFrame.cpp:565-569
                                              : ORBGPU_COVIS_CULL_CULLED;
                if (verdict == ORBGPU_COVIS_CULL_CULLED) {
                    ++n_culled;
                    if (tid == 0) {
                        unsigned h = cull_hash(k);
                        while (s_tab[h] >= 0) h = (h + 1) & (kCullHash - 1);
                        s_tab[h] = k;
                    }
                } else if (verdict == ORBGPU_COVIS_CULL_TO_BE_ERASED) {
                    ++n_tbe;
                }
            }
            if (tid == 0) {
                s_verdict[e] = verdict;
                s_mps[e] = n_mps;
                s_red[e] = n_red;
            }
            __syncthreads();  // the culled set, and the counters before they are cleared
        }
        __syncthreads();
        if (bad) {
            status = ORBGPU_COVIS_BAD_JOB;
            n_list = n_culled = n_tbe = 0;
        }
    }
    const bool ok = status == ORBGPU_COVIS_OK;
    for (int e = tid; e < list_stride; e += kThreads) {
        const bool in_list = ok && e < n_list;
        if (in_list) {
            vrow[e].kf = s_list[e];
            vrow[e].n_mps = s_mps[e];
            vrow[e].n_redundant = s_red[e];
            vrow[e].verdict = s_verdict[e];
        }
        crow[e] = in_list && s_verdict[e] == ORBGPU_COVIS_CULL_CULLED ? s_list[e] : -1;
    }
    if (tid == 0) {
        orbgpu_covis_cull_result& r = results[job];
        r.status = status;
        r.n_list = n_list;
        r.n_culled = n_culled;
        r.n_to_be_erased = n_tbe;
        r.pad[0] = r.pad[1] = r.pad[2] = r.pad[3] = 0;
    }
}

const char* graph_error(const orbgpu_covis_graph* g) {
    if (!g) return "graph is NULL";
    if (g->n_kf < 0) return "graph n_kf is negative";
    if (g->conn_stride < 1 || g->conn_stride > ORBGPU_COVIS_MAX_STRIDE) return "conn_stride outside 1..ORBGPU_COVIS_MAX_STRIDE";
    if ((long long)g->n_kf * g->conn_stride > 0x7fffffffLL) return "n_kf * conn_stride overflows";
    if (g->n_kf > 0 && (!g->n_conn || !g->conn_kf || !g->conn_w || !g->n_ord || !g->ord_kf || !g->ord_w || !g->covis10))
        return "an array of the graph is NULL";
    return nullptr;
}

// the first mirror as the two new calls read it; no pointer is dereferenced
const char* mirror_error(const orbgpu_map_mirror* m, const orbgpu_covis_graph* g) {
    if (!m) return "mirror is NULL";
    if (m->n_kf < 0 || m->n_pt < 0 || m->n_slots_total < 0 || m->n_obs_total < 0) return "a count of the mirror is negative";
    if (m->n_kf != g->n_kf) return "mirror n_kf differs from the graph's";
    if (m->n_kf > 0 && (!m->slot_offset || !m->n_slots)) return "a keyframe array of the mirror is NULL";
    if (m->n_slots_total > 0 && !m->slots) return "mirror slots is NULL";
    if (m->n_pt > 0 && (!m->pt_flags || !m->obs_offset || !m->n_obs)) return "a point array of the mirror is NULL";
    if (m->n_obs_total > 0 && !m->obs) return "mirror obs is NULL";
    return nullptr;
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

int orbgpu_covis_erase_keyframes_batch_device(int n, const int* d_kfs, const orbgpu_covis_graph* graph, int* d_status,
                                              void* stream) {
    if (n < 0) return fail(ORBGPU_ERR_ARG, "n is negative");
    if (n > 0 && (!d_kfs || !d_status)) return fail(ORBGPU_ERR_ARG, "a NULL pointer with n > 0");
    if (n > 0 || graph)
        if (const char* e = graph_error(graph)) return fail(ORBGPU_ERR_ARG, e);
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(erase_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, n, d_kfs, *graph, d_status);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

size_t orbgpu_covis_update_workspace_bytes(int n, int n_kf) {
    if (n < 0 || n_kf < 0) return 0;
    const long long ints = update_ws_ints(n, n_kf);
    return ints > 0x7fffffffLL ? 0 : (size_t)ints * sizeof(int);
}

int orbgpu_covis_update_connections_batch_device(int n, const int* d_kfs, const orbgpu_map_mirror* mirror,
                                                 const orbgpu_covis_graph* graph, void* d_workspace, size_t workspace_bytes,
                                                 orbgpu_covis_update_result* d_results, void* stream) {
    if (n < 0) return fail(ORBGPU_ERR_ARG, "n is negative");
    if (n > 0 && (!d_kfs || !d_results)) return fail(ORBGPU_ERR_ARG, "a NULL pointer with n > 0");
    if (n > 0 || graph)
        if (const char* e = graph_error(graph)) return fail(ORBGPU_ERR_ARG, e);
    if (n > 0 || (graph && mirror))
        if (const char* e = mirror_error(mirror, graph)) return fail(ORBGPU_ERR_ARG, e);
    if (n == 0) return ORBGPU_OK;
    const size_t need = orbgpu_covis_update_workspace_bytes(n, graph->n_kf);
    if (need == 0) return fail(ORBGPU_ERR_ARG, "n * n_kf overflows");
    if (!d_workspace || workspace_bytes < need) return fail(ORBGPU_ERR_ARG, "the workspace is NULL or short");
    if (int rc = check_device()) return rc;
    const UpdateWs W = update_ws(d_workspace, n, graph->n_kf);
    const long long ints = update_ws_ints(n, graph->n_kf);
    const hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    const int clear_blocks = (int)((ints + kCountThreads - 1) / kCountThreads < 2048 ? (ints + kCountThreads - 1) / kCountThreads : 2048);
    hipLaunchKernelGGL(update_clear_kernel, dim3(clear_blocks), dim3(kCountThreads), 0, s, W.rank_of, graph->n_kf, ints);
    if (mirror->kf_by_rank) {
        const int blocks = (graph->n_kf + kCountThreads - 1) / kCountThreads;
        hipLaunchKernelGGL(update_rank_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(kCountThreads), 0, s, mirror->kf_by_rank,
                           graph->n_kf, W);
    }
    hipLaunchKernelGGL(update_count_kernel, dim3(n, kCountChunks), dim3(kCountThreads), 0, s, d_kfs, *mirror, W);
    hipLaunchKernelGGL(update_apply_kernel, dim3(1), dim3(kThreads), 0, s, n, d_kfs, mirror->kf_by_rank, *graph, W, d_results);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

int orbgpu_covis_keyframe_culling_batch_device(int n, const orbgpu_covis_cull_job* d_jobs, const orbgpu_map_mirror* mirror,
                                               const orbgpu_map_mirror_ba* mirror_ba, const orbgpu_map_mirror_cull* mirror_cull,
                                               const orbgpu_covis_graph* graph, int list_stride,
                                               orbgpu_covis_cull_result* d_results, orbgpu_covis_cull_verdict* d_verdicts,
                                               int* d_culled, void* stream) {
    if (n < 0) return fail(ORBGPU_ERR_ARG, "n is negative");
    if (list_stride < 1) return fail(ORBGPU_ERR_ARG, "list_stride is not positive");
    if ((long long)n * list_stride > 0x7fffffffLL) return fail(ORBGPU_ERR_ARG, "n * list_stride overflows");
    if (n > 0 && (!d_jobs || !d_results || !d_verdicts || !d_culled)) return fail(ORBGPU_ERR_ARG, "a NULL pointer with n > 0");
    if (n > 0 || graph)
        if (const char* e = graph_error(graph)) return fail(ORBGPU_ERR_ARG, e);
    if (n > 0 || (graph && mirror))
        if (const char* e = mirror_error(mirror, graph)) return fail(ORBGPU_ERR_ARG, e);
    if (n > 0 || (mirror && mirror_ba && mirror_cull)) {
        if (!mirror_ba || !mirror_cull) return fail(ORBGPU_ERR_ARG, "mirror_ba or mirror_cull is NULL");
        if (mirror->n_kf > 0 && (!mirror_ba->kf_first || !mirror_cull->kf_th_depth || !mirror_cull->kf_not_erase))
            return fail(ORBGPU_ERR_ARG, "a keyframe array of mirror_ba or mirror_cull is NULL");
        if (mirror->n_slots_total > 0 && (!mirror_ba->kp_obs || !mirror_cull->kp_octave || !mirror_cull->kp_depth))
            return fail(ORBGPU_ERR_ARG, "a slot array of mirror_ba or mirror_cull is NULL");
        if (mirror->n_obs_total > 0 && !mirror_ba->obs_idx) return fail(ORBGPU_ERR_ARG, "mirror_ba obs_idx is NULL");
    }
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cull_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, d_jobs, *mirror, *mirror_ba, *mirror_cull,
                       *graph, list_stride, d_results, d_verdicts, d_culled);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

}  // extern "C"
