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

const char* graph_error(const orbgpu_covis_graph* g) {
    if (!g) return "graph is NULL";
    if (g->n_kf < 0) return "graph n_kf is negative";
    if (g->conn_stride < 1 || g->conn_stride > ORBGPU_COVIS_MAX_STRIDE) return "conn_stride outside 1..ORBGPU_COVIS_MAX_STRIDE";
    if ((long long)g->n_kf * g->conn_stride > 0x7fffffffLL) return "n_kf * conn_stride overflows";
    if (g->n_kf > 0 && (!g->n_conn || !g->conn_kf || !g->conn_w || !g->n_ord || !g->ord_kf || !g->ord_w || !g->covis10))
        return "an array of the graph is NULL";
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

}  // extern "C"
