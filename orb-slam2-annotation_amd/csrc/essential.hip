// essential.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:905-1200)
// for ONE 7-dof pose graph spread over the whole chip
// (include/orbgpu_essential.h): Sim3 vertices, EdgeSim3 with its logarithm, the
// numeric Jacobians of both ends, the non-robust quadratic form, the active set
// of initializeOptimization(0), g2o's Levenberg-Marquardt from lambda = 1e-16
// and the write-out (SE3 recovery, MapPoint correction), as one launch per
// phase.  There are no points in the graph and no Schur complement: the system
// over the free active vertices is dense and is solved by chol_blocked.h.
// tests/essential_ref.py is the same arithmetic, expression for expression.
// The Sim3 algebra is sim3opt_device.h's and sim3_log_device.h's, the LM
// decisions are lm_runtime.h's; the control block, the host record, the ordered
// sums and the bodies of the begin and judge kernels are wholechip_lm.h's,
// shared with globalba.hip.
//
// The calling thread drives the loop as globalba.hip's does: a phase that needs
// the previous one complete is the next launch on the stream; no kernel
// synchronises with another workgroup, spins on memory or is launched
// cooperatively.  A one-lane judge kernel advances lm::Run in the workspace and
// copies its decisions into a coherent pinned host record; the host
// synchronises the stream once per trial: at most n_iterations (1 + 10) passes
// on any input.
//
// Every sum has one owner that adds its terms in a fixed order, and there are no
// floating-point atomics:
//   an edge's A^T A, A^T B, B^T B,  one lane per entry, over the 7 rows of the error ascending
//     A^T (-e), B^T (-e)
//   entry r of a vertex's b          one lane, over the vertex's active edges ascending (a vertex-major
//                                    edge list built once per call by a ballot scan)
//   entry of a diagonal block        one lane, over the vertex's active edges ascending
//   entry of an off-diagonal block   one lane, over the active edges between the two vertices ascending
//                                    (found in the shorter of the two vertices' lists), transposing an
//                                    edge that runs the other way
//   factor, back-substitution        chol_blocked.h
//   chi2, computeScale               per-workgroup partial sums in lane order (16 lanes add 16 values
//                                    each, lane 0 the 16 sums), added in workgroup order by the one lane
//                                    of the begin / judge kernel
// Loop bounds are counts of the index structure, never floating-point values.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/orbgpu_essential.h"
#include "chol_blocked.h"
#include "host_common.h"
#include "host_ctx.h"
#include "sim3_log_device.h"
#include "wholechip_lm.h"

namespace {

namespace lm = orbgpu::lm;
namespace chol = orbgpu::chol;
namespace wc = orbgpu::wholechip;
using wc::block_total;
using wc::blocks_for;
using wc::global_tid;
using wc::HostRec;
using wc::kCtlBytes;
using orbgpu::sim3opt::Sim3;
using orbgpu::sim3opt::sim3_exp;
using orbgpu::sim3opt::sim3_inverse;
using orbgpu::sim3opt::sim3_log;
using orbgpu::sim3opt::sim3_map;
using orbgpu::sim3opt::sim3_mul;

constexpr int kThreads = 256;
constexpr double kDelta = 1e-9;                   // base_binary_edge.hpp:147
constexpr double kScalar = 1.0 / (2 * kDelta);    // :148
constexpr double kLambdaInit = 1e-16;             // Optimizer.cpp:922

// doubles per vertex and edge in the workspace, and where each field starts.  A Sim3 is 8 doubles
// (q, t, s).  V_PERT: the 14 perturbed estimates, 2 d + (0: +delta, 1: -delta); V_INV: the inverses
// of the estimate (0) and of the 14 (1 + ...)
constexpr int V_SCW = 0, V_EST = 8, V_TRIAL = 16, V_B = 24, V_PERT = 31, V_INV = V_PERT + 14 * 8, kVertD = V_INV + 15 * 8;
// E_A, E_B: the Jacobians, row-major [error row][column]
constexpr int E_MEAS = 0, E_ERR = 8, E_A = 15, E_B = E_A + 49, E_ATA = E_B + 49, E_ATB = E_ATA + 49,
              E_BTB = E_ATB + 49, E_ATE = E_BTB + 49, E_BTE = E_ATE + 7, kEdgeD = E_BTE + 7;
constexpr int kEdgeProducts = 3 * 49 + 2 * 7;
// ints per vertex
constexpr int IV_HIDX = 0, IV_HLIST = 1, IV_START = 2, IV_COUNT = 3, IV_FREE = 4, kVertI = 5;

using Ctl = wc::CtlBase;  // nothing of its own

struct Layout {
    size_t N, E, n_max;                          // n_max = 7 N
    size_t vert_d, edge_d, sys_d, x_d, chi_d, scale_d;  // in doubles, after the control block
    size_t n_chi, n_scale;
    size_t ints;                                 // byte offset of the ints
    size_t vert_i, active_i, list_i;
    size_t bytes;                                // 0: does not fit
};

inline Layout make_layout(int n_kf, int n_edges) {
    Layout l;
    std::memset(&l, 0, sizeof(l));
    typedef unsigned __int128 u128;
    const u128 N = (u128)n_kf, E = (u128)n_edges, n = 7 * N;
    const u128 n_chi = (E + kThreads - 1) / kThreads, n_scale = (N + kThreads - 1) / kThreads;
    const u128 doubles = kVertD * N + kEdgeD * E + (n + 1) * n + n + n_chi + n_scale;
    const u128 ints = kVertI * N + E + 2 * E;
    const u128 bytes = kCtlBytes + doubles * 8 + ((ints * 4 + 7) / 8) * 8 + 8;
    if (bytes > (u128)(SIZE_MAX / 2)) return l;
    l.N = (size_t)N, l.E = (size_t)E, l.n_max = (size_t)n;
    l.n_chi = (size_t)n_chi, l.n_scale = (size_t)n_scale;
    l.vert_d = 0;
    l.edge_d = l.vert_d + kVertD * l.N;
    l.sys_d = l.edge_d + kEdgeD * l.E;
    l.x_d = l.sys_d + (l.n_max + 1) * l.n_max;
    l.chi_d = l.x_d + l.n_max;
    l.scale_d = l.chi_d + l.n_chi;
    l.ints = kCtlBytes + (size_t)doubles * 8;
    l.vert_i = 0;
    l.active_i = l.vert_i + kVertI * l.N;
    l.list_i = l.active_i + l.E;
    l.bytes = (size_t)bytes;
    return l;
}

// what every kernel gets
struct Args {
    int N, E, M, fix_scale;
    const float *Tcw, *Xw;
    const uint8_t *has_c, *has_nc, *fixed, *kind;
    const double *Sc, *Snc;
    const int *ei, *ej, *point_ref;
    double* Scw_out;
    float *Tcw_out, *Xw_out;
    Ctl* ctl;
    HostRec* rec;
    double *wv, *we, *S, *x, *chi_part, *scale_part;
    int *iv, *active, *list;
    int n_chi, n_scale;
};

// the view chol_blocked.h's kernels take
struct SystemView {
    double *S, *x;
    int* fail;
    const int* nf;
    __device__ size_t n() const { return 7 * (size_t)*nf; }
};

#define VD(f, v) A.wv[(size_t)(f) * A.N + (v)]
#define ED(f, e) A.we[(size_t)(f) * A.E + (e)]
#define VI(f, v) A.iv[(size_t)(f) * A.N + (v)]

__device__ inline void load_sim3(const Args& A, int field, int v, Sim3& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s.q[k] = VD(field + k, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.t[k] = VD(field + 4 + k, v);
    s.s = VD(field + 7, v);
}

__device__ inline void store_sim3(const Args& A, int field, int v, const Sim3& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) VD(field + k, v) = s.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) VD(field + 4 + k, v) = s.t[k];
    VD(field + 7, v) = s.s;
}

__device__ inline void load_rows8(const double* p, Sim3& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s.q[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s.t[k] = p[4 + k];
    s.s = p[7];
}

// EdgeSim3::computeError: (C * v1.estimate() * v2.estimate().inverse()).log()
__device__ inline void edge_error(const Sim3& C, const Sim3& Si, const Sim3& Sj_inv, double (&e)[7]) {
    Sim3 a, b;
    sim3_mul(C, Si, a);
    sim3_mul(a, Sj_inv, b);
    sim3_log(b, e);
}

__device__ inline double chi2_of(const double (&e)[7]) {
    double c = e[0] * e[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) c = c + e[k] * e[k];
    return c;
}

// ------------------------------------------------------------------ once per call: check and structure

// an edge index out of range, an edge from a keyframe to itself or a point_ref past the keyframes:
// nothing else may index with these arrays
__global__ __launch_bounds__(kThreads) void eg_check(Args A) {
    const size_t i = global_tid();
    if (i < (size_t)A.E) {
        const int a = A.ei[i], b = A.ej[i];
        if (a < 0 || a >= A.N || b < 0 || b >= A.N || a == b) A.ctl->bad = 1;
    }
    if (i < (size_t)A.M && A.point_ref[i] >= A.N) A.ctl->bad = 1;
}

// vScw of every keyframe (:951-966), which is its first estimate; the counters cleared
__global__ __launch_bounds__(kThreads) void eg_init(Args A) {
    if (A.ctl->bad) return;
    const size_t i = global_tid();
    if (i >= (size_t)A.N) return;
    const int v = (int)i;
    Sim3 s;
    if (A.has_c[v]) {
        load_rows8(A.Sc + 8 * i, s);
    } else {  // g2o::Sim3(Rcw, tcw, 1.0): Quaterniond(Matrix3d), not normalised
        const float* Tp = A.Tcw + 12 * i;
        double R[9];
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 3; ++col) R[3 * r + col] = (double)Tp[4 * r + col];
        lm::quat_from_R(R, s.q);
        for (int r = 0; r < 3; ++r) s.t[r] = (double)Tp[4 * r + 3];
        s.s = 1.0;
    }
    store_sim3(A, V_SCW, v, s);
    store_sim3(A, V_EST, v, s);
    VI(IV_COUNT, v) = 0;
}

// every edge's measurement (:994-1005, :1029-1057) and whether it is active; the number of active
// edges of every vertex (integer atomics)
__global__ __launch_bounds__(kThreads) void eg_measure(Args A) {
    if (A.ctl->bad) return;
    const size_t gi = global_tid();
    if (gi >= (size_t)A.E) return;
    const int e = (int)gi, i = A.ei[e], j = A.ej[e];
    Sim3 Si, Sj, Swi, Sji;
    const bool normal = A.kind[e] != 0;
    if (normal && A.has_nc[i])
        load_rows8(A.Snc + 8 * (size_t)i, Si);
    else
        load_sim3(A, V_SCW, i, Si);
    if (normal && A.has_nc[j])
        load_rows8(A.Snc + 8 * (size_t)j, Sj);
    else
        load_sim3(A, V_SCW, j, Sj);
    sim3_inverse(Si, Swi);
    sim3_mul(Sj, Swi, Sji);
#pragma unroll
    for (int k = 0; k < 4; ++k) ED(E_MEAS + k, e) = Sji.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ED(E_MEAS + 4 + k, e) = Sji.t[k];
    ED(E_MEAS + 7, e) = Sji.s;
    const int active = !(A.fixed[i] && A.fixed[j]);  // sparse_optimizer.cpp:234
    A.active[e] = active;
    if (active) {
        atomicAdd(&VI(IV_COUNT, i), 1);
        atomicAdd(&VI(IV_COUNT, j), 1);
        atomicAdd(&A.ctl->n_active, 1);
    }
}

// where each vertex's edge list starts, which vertices are free, their order in the system; one lane
__global__ void eg_scan(Args A) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    HostRec* rec = A.rec;
    rec->bad = A.ctl->bad;
    if (A.ctl->bad) {
        rec->nf = 0, rec->n_active = 0;
        __threadfence_system();
        return;
    }
    int s = 0, nf = 0;
    for (int v = 0; v < A.N; ++v) {
        const int count = VI(IV_COUNT, v);
        VI(IV_START, v) = s;
        s += count;
        const int is_free = count > 0 && !A.fixed[v];
        VI(IV_FREE, v) = is_free;
        VI(IV_HIDX, v) = -1;
        if (is_free) VI(IV_HIDX, v) = nf, VI(IV_HLIST, nf) = v, ++nf;
    }
    A.ctl->nf = nf;
    rec->nf = nf, rec->n_active = A.ctl->n_active;
    __threadfence_system();
}

// the vertex-major list of active edges, ascending: one wave per vertex scans the edges 64 at a time
__global__ __launch_bounds__(kThreads) void eg_lists(Args A) {
    if (A.ctl->bad) return;
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (v >= A.N) return;  // a whole wave
    int before = VI(IV_START, v);
    for (int i0 = 0; i0 < A.E; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < A.E && A.active[i] && (A.ei[i] == v || A.ej[i] == v);
        const unsigned long long mask = __ballot(mine);
        if (mine) A.list[before + (int)__popcll(mask & ((1ull << lane) - 1))] = i;
        before += (int)__popcll(mask);
    }
}

// ------------------------------------------------------------------ per iteration: the build

// the inverse of every estimate, and of every free active vertex the 14 estimates
// oplus(+-delta e_d) = Sim3(u) * estimate with their inverses; one lane per (vertex, 1 + 14)
__global__ __launch_bounds__(kThreads) void eg_perturb(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.N * 15) return;
    const int v = (int)(gi / 15), k = (int)(gi % 15);
    Sim3 est, inv;
    load_sim3(A, V_EST, v, est);
    if (k == 0) {
        sim3_inverse(est, inv);
        store_sim3(A, V_INV, v, inv);
        return;
    }
    if (!VI(IV_FREE, v)) return;
    const int d = (k - 1) >> 1;
    const double step = ((k - 1) & 1) ? -kDelta : kDelta;
    double u[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) u[c] = c == d ? step : 0.0;
    if (A.fix_scale) u[6] = 0.0;  // VertexSim3Expmap::oplusImpl
    Sim3 ex, p;
    sim3_exp(u, ex);
    sim3_mul(ex, est, p);
    sim3_inverse(p, inv);
    store_sim3(A, V_PERT + 8 * (k - 1), v, p);
    store_sim3(A, V_INV + 8 * k, v, inv);
}

// computeActiveErrors at the estimates (kBuild: the error is kept) or at the trial; the workgroup's chi2
// goes to chi_part[blockIdx.x]
template <bool kBuild>
__global__ __launch_bounds__(kThreads) void eg_error(Args A) {
    __shared__ double s_val[kThreads];
    __shared__ double s_row[16];
    if (!kBuild && A.ctl->fail) return;
    const size_t gi = global_tid();
    double chi2 = 0.0;
    if (gi < (size_t)A.E && A.active[gi]) {
        const int e = (int)gi;
        Sim3 C, Si, Sj, Sj_inv;
#pragma unroll
        for (int k = 0; k < 4; ++k) C.q[k] = ED(E_MEAS + k, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) C.t[k] = ED(E_MEAS + 4 + k, e);
        C.s = ED(E_MEAS + 7, e);
        load_sim3(A, kBuild ? V_EST : V_TRIAL, A.ei[e], Si);
        load_sim3(A, kBuild ? V_EST : V_TRIAL, A.ej[e], Sj);
        sim3_inverse(Sj, Sj_inv);
        double err[7];
        edge_error(C, Si, Sj_inv, err);
        chi2 = chi2_of(err);
        if (kBuild) {
#pragma unroll
            for (int k = 0; k < 7; ++k) ED(E_ERR + k, e) = err[k];
        }
    }
    const double total = block_total(chi2, s_val, s_row);
    if (threadIdx.x == 0) A.chi_part[blockIdx.x] = total;
}

// BaseBinaryEdge::linearizeOplus: one lane per (edge, 14): column d of A (vertex i perturbed) or of B
// (vertex j perturbed); the columns of a fixed end are zero and never read
__global__ __launch_bounds__(kThreads) void eg_jacobian(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.E * 14) return;
    const int e = (int)(gi / 14), c = (int)(gi % 14);
    if (!A.active[e]) return;
    const int side = c / 7, d = c % 7;
    const int i = A.ei[e], j = A.ej[e];
    const int field = side ? E_B : E_A;
    if (A.fixed[side ? j : i]) {
        for (int r = 0; r < 7; ++r) ED(field + 7 * r + d, e) = 0.0;
        return;
    }
    Sim3 C, Si, Sj_inv;
#pragma unroll
    for (int k = 0; k < 4; ++k) C.q[k] = ED(E_MEAS + k, e);
#pragma unroll
    for (int k = 0; k < 3; ++k) C.t[k] = ED(E_MEAS + 4 + k, e);
    C.s = ED(E_MEAS + 7, e);
    double ep[7], em[7];
    if (side == 0) {
        load_sim3(A, V_INV, j, Sj_inv);
        load_sim3(A, V_PERT + 8 * (2 * d), i, Si);
        edge_error(C, Si, Sj_inv, ep);
        load_sim3(A, V_PERT + 8 * (2 * d + 1), i, Si);
        edge_error(C, Si, Sj_inv, em);
    } else {
        load_sim3(A, V_EST, i, Si);
        load_sim3(A, V_INV + 8 * (1 + 2 * d), j, Sj_inv);
        edge_error(C, Si, Sj_inv, ep);
        load_sim3(A, V_INV + 8 * (2 + 2 * d), j, Sj_inv);
        edge_error(C, Si, Sj_inv, em);
    }
#pragma unroll
    for (int r = 0; r < 7; ++r) ED(field + 7 * r + d, e) = (ep[r] - em[r]) * kScalar;
}

// the edge's terms of the quadratic form, one lane per entry: A^T A, A^T B, B^T B (49 each, row-major),
// A^T (-e), B^T (-e); every entry is its sum over the 7 rows of the error in ascending order
__global__ __launch_bounds__(kThreads) void eg_products(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.E * kEdgeProducts) return;
    const int e = (int)(gi / kEdgeProducts), v = (int)(gi % kEdgeProducts);
    if (!A.active[e]) return;
    if (v < 3 * 49) {
        const int which = v / 49, r = (v % 49) / 7, c = v % 7;
        const int left = which == 2 ? E_B : E_A, right = which == 0 ? E_A : E_B;
        double acc = ED(left + r, e) * ED(right + c, e);
        for (int k = 1; k < 7; ++k) acc = acc + ED(left + 7 * k + r, e) * ED(right + 7 * k + c, e);
        ED(E_ATA + v, e) = acc;
        return;
    }
    const int w = v - 3 * 49, side = w / 7, r = w % 7;
    const int left = side ? E_B : E_A;
    double acc = ED(left + r, e) * (-ED(E_ERR, e));
    for (int k = 1; k < 7; ++k) acc = acc + ED(left + 7 * k + r, e) * (-ED(E_ERR + k, e));
    ED(E_ATE + w, e) = acc;
}

// b of every free active vertex: one lane per entry, over the vertex's active edges ascending
__global__ __launch_bounds__(kThreads) void eg_vertex_b(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.N * 7) return;
    const int v = (int)(gi / 7), r = (int)(gi % 7);
    if (!VI(IV_FREE, v)) return;
    const int start = VI(IV_START, v), count = VI(IV_COUNT, v);
    double acc = 0.0;
    for (int s = 0; s < count; ++s) {
        const int e = A.list[start + s];
        acc += ED((A.ei[e] == v ? E_ATE : E_BTE) + r, e);
    }
    VD(V_B + r, v) = acc;
}

// the iteration begins: chi2 at the kept estimates; lambda = 1e-16 in the first
__global__ void eg_begin(Args A, int first) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    wc::begin_iteration(*A.ctl, A.chi_part, A.n_chi, first,
                        [](lm::Run& run) { lm::run_init_lambda_user(run, kLambdaInit); });
}

// ------------------------------------------------------------------ per trial

// the lower triangle of H + lambda I, rows of n = 7 nf doubles, and b as row n: one lane per entry.
// Entry (row, col), col <= row: row = 7 hb + s, col = 7 ha + r.
__global__ __launch_bounds__(kThreads) void eg_assemble(Args A) {
    const int nf = A.ctl->nf;
    const size_t n = 7 * (size_t)nf;
    const size_t gi = global_tid();
    if (gi >= (n + 1) * n) return;
    const size_t row = gi / n, col = gi % n;
    const int ha = (int)(col / 7), r = (int)(col % 7);
    const int va = VI(IV_HLIST, ha);
    if (row == n) {
        A.S[gi] = VD(V_B + r, va);
        return;
    }
    if (col > row) return;
    const int hb = (int)(row / 7), s = (int)(row % 7);
    const int vb = VI(IV_HLIST, hb);
    double acc = 0.0;
    if (ha == hb) {
        const int start = VI(IV_START, va), count = VI(IV_COUNT, va);
        for (int k = 0; k < count; ++k) {
            const int e = A.list[start + k];
            acc += ED((A.ei[e] == va ? E_ATA : E_BTB) + 7 * s + r, e);
        }
        if (s == r) acc = acc + A.ctl->run.lambda;
    } else {
        const int scan = VI(IV_COUNT, va) <= VI(IV_COUNT, vb) ? va : vb;
        const int start = VI(IV_START, scan), count = VI(IV_COUNT, scan);
        for (int k = 0; k < count; ++k) {
            const int e = A.list[start + k], i = A.ei[e], j = A.ej[e];
            if (i == va && j == vb)
                acc += ED(E_ATB + 7 * r + s, e);
            else if (i == vb && j == va)
                acc += ED(E_ATB + 7 * s + r, e);  // the edge runs the other way: its block transposed
        }
    }
    A.S[gi] = acc;
}

// trial = oplus(x) on the estimates, one lane per vertex, and the vertex's terms of computeScale's
// sum; the workgroup's sum goes to scale_part[blockIdx.x]
__global__ __launch_bounds__(kThreads) void eg_trial(Args A) {
    __shared__ double s_val[kThreads];
    __shared__ double s_row[16];
    const size_t gi = global_tid();
    const bool ok = !A.ctl->fail;
    const double lambda = A.ctl->run.lambda;
    double acc = 0.0;
    if (gi < (size_t)A.N) {
        const int v = (int)gi;
        Sim3 est;
        load_sim3(A, V_EST, v, est);
        if (ok && VI(IV_FREE, v)) {
            const double* xp = A.x + 7 * (size_t)VI(IV_HIDX, v);
            double x[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) x[k] = xp[k];
            if (A.fix_scale) x[6] = 0.0;  // oplusImpl zeroes the solver's own x[6]: computeScale sees it
            Sim3 ex, trial;
            sim3_exp(x, ex);
            sim3_mul(ex, est, trial);
            store_sim3(A, V_TRIAL, v, trial);
#pragma unroll
            for (int k = 0; k < 7; ++k) acc = acc + x[k] * (lambda * x[k] + VD(V_B + k, v));
        } else {
            store_sim3(A, V_TRIAL, v, est);
        }
    }
    const double total = block_total(acc, s_val, s_row);
    if (threadIdx.x == 0) A.scale_part[blockIdx.x] = total;
}

// OptimizationAlgorithmLevenberg::solve's decisions after a trial, by one lane; the host reads rec
__global__ void eg_judge(Args A, int max_iter) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    wc::judge(*A.ctl, A.rec, A.chi_part, A.n_chi, A.scale_part, A.n_scale, max_iter);
}

// an accepted trial becomes the estimate
__global__ __launch_bounds__(kThreads) void eg_accept(Args A) {
    const size_t gi = global_tid();
    if (gi < (size_t)A.N * 8) A.wv[(size_t)V_EST * A.N + gi] = A.wv[(size_t)V_TRIAL * A.N + gi];
}

// ------------------------------------------------------------------ the write-out (:1144-1199)

// per keyframe the final Sim3 and Tiw = [R | t / s]; per point with a reference keyframe r,
// vCorrectedSwc[r].map(vScw[r].map(Xw)); a point without one keeps its bits
__global__ __launch_bounds__(kThreads) void eg_write(Args A) {
    const size_t gi = global_tid();
    if (gi < (size_t)A.N) {
        Sim3 est;
        load_sim3(A, V_EST, (int)gi, est);
        double* so = A.Scw_out + 8 * gi;
        for (int k = 0; k < 4; ++k) so[k] = est.q[k];
        for (int k = 0; k < 3; ++k) so[4 + k] = est.t[k];
        so[7] = est.s;
        const double inv_s = 1.0 / est.s;  // eigt *= (1./s)
        const double t[3] = {est.t[0] * inv_s, est.t[1] * inv_s, est.t[2] * inv_s};
        lm::write_T16(est.q, t, 1.0, A.Tcw_out + 16 * gi);
    }
    if (gi < (size_t)A.M) {
        const int r = A.point_ref[gi];
        const float* X = A.Xw + 3 * gi;
        float* Xo = A.Xw_out + 3 * gi;
        if (r < 0) {
            for (int k = 0; k < 3; ++k) Xo[k] = X[k];
        } else {
            Sim3 Srw, est, Swr;
            load_sim3(A, V_SCW, r, Srw);
            load_sim3(A, V_EST, r, est);
            sim3_inverse(est, Swr);
            const double p[3] = {(double)X[0], (double)X[1], (double)X[2]};
            double mid[3], out[3];
            sim3_map(Srw, p, mid);
            sim3_map(Swr, mid, out);
            for (int k = 0; k < 3; ++k) Xo[k] = (float)out[k];
        }
    }
}

#undef VD
#undef ED
#undef VI

// ------------------------------------------------------------------ host

int check_args(int n_kf, int n_edges, int n_points, int n_iterations, bool kf_arrays, bool edge_arrays,
               bool point_arrays, bool result) {
    using orbgpu::fail;
    if (n_kf < 0 || n_edges < 0 || n_points < 0 || n_iterations < 0)
        return fail(ORBGPU_ERR_ARG, "negative count or n_iterations");
    if (!result) return fail(ORBGPU_ERR_ARG, "null result");
    if (n_kf > 0 && !kf_arrays) return fail(ORBGPU_ERR_ARG, "null keyframe array");
    if (n_edges > 0 && !edge_arrays) return fail(ORBGPU_ERR_ARG, "null edge array");
    if (n_points > 0 && !point_arrays) return fail(ORBGPU_ERR_ARG, "null point array");
    return ORBGPU_OK;
}

}  // namespace

extern "C" size_t orbgpu_essential_graph_workspace_bytes(int n_kf, int n_edges, int n_points) {
    if (n_kf < 0 || n_edges < 0 || n_points < 0) return 0;
    return make_layout(n_kf, n_edges).bytes;
}

extern "C" int orbgpu_optimize_essential_graph_device(
    int n_kf, int n_edges, int n_points, const float* d_Tcw, const uint8_t* d_has_corrected, const double* d_Scorrected,
    const uint8_t* d_has_noncorrected, const double* d_Snoncorrected, const uint8_t* d_fixed, const int* d_edge_i,
    const int* d_edge_j, const uint8_t* d_edge_kind, const float* d_Xw, const int* d_point_ref, int fix_scale,
    int n_iterations, double* d_Scw_out, float* d_Tcw_out, float* d_Xw_out, orbgpu_eg_result* result,
    void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_args(n_kf, n_edges, n_points, n_iterations,
                            d_Tcw && d_has_corrected && d_Scorrected && d_has_noncorrected && d_Snoncorrected &&
                                d_fixed && d_Scw_out && d_Tcw_out,
                            d_edge_i && d_edge_j && d_edge_kind, d_Xw && d_point_ref && d_Xw_out, result))
        return rc;
    const Layout L = make_layout(n_kf, n_edges);
    if (!d_workspace || ((uintptr_t)d_workspace & 7) || L.bytes == 0 || workspace_bytes < L.bytes)
        return orbgpu::fail(ORBGPU_ERR_ARG, "null, misaligned or too small workspace");
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    std::memset(result, 0, sizeof(*result));
    HostRec* rec;
    if (int rc = wc::host_rec(&rec)) return rc;
    std::memset(rec, 0, sizeof(*rec));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    Args a;
    a.N = n_kf, a.E = n_edges, a.M = n_points, a.fix_scale = fix_scale ? 1 : 0;
    a.Tcw = d_Tcw, a.Xw = d_Xw, a.has_c = d_has_corrected, a.has_nc = d_has_noncorrected, a.fixed = d_fixed;
    a.kind = d_edge_kind, a.Sc = d_Scorrected, a.Snc = d_Snoncorrected, a.ei = d_edge_i, a.ej = d_edge_j;
    a.point_ref = d_point_ref, a.Scw_out = d_Scw_out, a.Tcw_out = d_Tcw_out, a.Xw_out = d_Xw_out;
    uint8_t* base = static_cast<uint8_t*>(d_workspace);
    a.ctl = reinterpret_cast<Ctl*>(base);
    a.rec = rec;
    double* d = reinterpret_cast<double*>(base + kCtlBytes);
    a.wv = d + L.vert_d, a.we = d + L.edge_d, a.S = d + L.sys_d, a.x = d + L.x_d;
    a.chi_part = d + L.chi_d, a.scale_part = d + L.scale_d;
    int* ints = reinterpret_cast<int*>(base + L.ints);
    a.iv = ints + L.vert_i, a.active = ints + L.active_i, a.list = ints + L.list_i;
    a.n_chi = (int)L.n_chi, a.n_scale = (int)L.n_scale;
    SystemView view;
    view.S = a.S, view.x = a.x, view.fail = &a.ctl->fail, view.nf = &a.ctl->nf;

    const size_t N = L.N, E = L.E, M = (size_t)n_points;
    const dim3 T(kThreads);
    // once per call: the check, the estimates and the structure; one synchronisation
    ORB_HIP(hipMemsetAsync(a.ctl, 0, kCtlBytes, st));
    if (E + M) ORB_LAUNCH(st, eg_check, dim3(blocks_for(E > M ? E : M)), T, a);
    if (N) ORB_LAUNCH(st, eg_init, dim3(blocks_for(N)), T, a);
    if (E) ORB_LAUNCH(st, eg_measure, dim3(blocks_for(E)), T, a);
    ORB_LAUNCH(st, eg_scan, dim3(1), dim3(64), a);
    if (E && N) ORB_LAUNCH(st, eg_lists, dim3(blocks_for(N, kThreads / 64)), T, a);
    ORB_HIP(hipStreamSynchronize(st));
    if (rec->bad) {
        result->status = -1;
        return ORBGPU_OK;
    }
    const int nf = rec->nf;
    const size_t n = 7 * (size_t)nf;
    result->n_free = nf, result->n_active_edges = rec->n_active;

    int iterations = 0;
    bool done = false;
    if (nf > 0) {  // optimize() does nothing without a free active vertex
        for (int it = 0; it < n_iterations && !done; ++it) {
            ORB_LAUNCH(st, eg_perturb, dim3(blocks_for(N * 15)), T, a);
            ORB_LAUNCH(st, eg_error<true>, dim3(blocks_for(E)), T, a);
            ORB_LAUNCH(st, eg_jacobian, dim3(blocks_for(E * 14)), T, a);
            ORB_LAUNCH(st, eg_products, dim3(blocks_for(E * kEdgeProducts)), T, a);
            ORB_LAUNCH(st, eg_vertex_b, dim3(blocks_for(N * 7)), T, a);
            ORB_LAUNCH(st, eg_begin, dim3(1), dim3(64), a, it == 0 ? 1 : 0);
            iterations = it + 1;
            for (int trial = 0; trial < lm::kMaxTrials; ++trial) {
                ORB_LAUNCH(st, eg_assemble, dim3(blocks_for((n + 1) * n)), T, a);
                ORB_HIP(chol::enqueue_solve(view, n, st));
                ORB_LAUNCH(st, eg_trial, dim3(blocks_for(N)), T, a);
                ORB_LAUNCH(st, eg_error<false>, dim3(blocks_for(E)), T, a);
                ORB_LAUNCH(st, eg_judge, dim3(1), dim3(64), a, n_iterations);
                ORB_HIP(hipStreamSynchronize(st));
                if (rec->accepted) ORB_LAUNCH(st, eg_accept, dim3(blocks_for(N * 8)), T, a);
                if (!rec->more) break;
            }
            // run_end_iteration also ends at iter >= n_iterations: the loop's own bound
            done = rec->done != 0;
        }
    }
    if (N + M) ORB_LAUNCH(st, eg_write, dim3(blocks_for(N > M ? N : M)), T, a);
    ORB_HIP(hipStreamSynchronize(st));
    result->iterations = iterations;
    result->rejected = rec->rejected;
    result->first_chi2 = rec->first_chi, result->last_chi2 = rec->chi, result->last_lambda = rec->lambda;
    return ORBGPU_OK;
}

extern "C" int orbgpu_optimize_essential_graph(int n_kf, int n_edges, int n_points, const float* Tcw,
                                               const uint8_t* has_corrected, const double* Scorrected,
                                               const uint8_t* has_noncorrected, const double* Snoncorrected,
                                               const uint8_t* fixed, const int* edge_i, const int* edge_j,
                                               const uint8_t* edge_kind, const float* Xw, const int* point_ref,
                                               int fix_scale, int n_iterations, double* Scw_out, float* Tcw_out,
                                               float* Xw_out, orbgpu_eg_result* result, void* d_workspace,
                                               size_t workspace_bytes) {
    using namespace orbgpu;
    int rc = check_args(n_kf, n_edges, n_points, n_iterations,
                        Tcw && has_corrected && Scorrected && has_noncorrected && Snoncorrected && fixed && Scw_out &&
                            Tcw_out,
                        edge_i && edge_j && edge_kind, Xw && point_ref && Xw_out, result);
    if (rc) return rc;
    for (int e = 0; e < n_edges; ++e) {
        const int i = edge_i[e], j = edge_j[e];
        if (i < 0 || i >= n_kf || j < 0 || j >= n_kf)
            return fail(ORBGPU_ERR_ARG, "edge " + std::to_string(e) + ": an index is out of range");
        if (i == j) return fail(ORBGPU_ERR_ARG, "edge " + std::to_string(e) + ": both ends are one keyframe");
    }
    for (int m = 0; m < n_points; ++m)
        if (point_ref[m] >= n_kf)
            return fail(ORBGPU_ERR_ARG, "point " + std::to_string(m) + ": point_ref is out of range");
    const size_t need = orbgpu_essential_graph_workspace_bytes(n_kf, n_edges, n_points);
    if (need == 0) return fail(ORBGPU_ERR_ARG, "the workspace does not fit a size_t");
    if (d_workspace && (((uintptr_t)d_workspace & 7) || workspace_bytes < need))
        return fail(ORBGPU_ERR_ARG, "misaligned or too small workspace");
    if ((rc = check_device())) return rc;
    DevBuf<uint8_t> own;
    if (!d_workspace) {
        if ((rc = dalloc(own, need))) return rc;
        d_workspace = own.get();
        workspace_bytes = need;
    }
    const size_t tn = (size_t)n_kf, te = (size_t)n_edges, tm = (size_t)n_points;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    HostCall call(*ctx);
    const float *dT, *dX;
    const uint8_t *dhc, *dhn, *dfix, *dkind;
    const double *dSc, *dSn;
    const int *dei, *dej, *dref;
    double* dSo;
    float *dTo, *dXo;
    rc = call.run([&](HostCall& A) {
        dSc = A.in(Scorrected, 8 * tn);
        dSn = A.in(Snoncorrected, 8 * tn);
        dSo = A.out<double>(8 * tn);
        dT = A.in(Tcw, 12 * tn);
        dhc = A.in(has_corrected, tn);
        dhn = A.in(has_noncorrected, tn);
        dfix = A.in(fixed, tn);
        dei = A.in(edge_i, te);
        dej = A.in(edge_j, te);
        dkind = A.in(edge_kind, te);
        dX = A.in(Xw, 3 * tm);
        dref = A.in(point_ref, tm);
        dTo = A.out<float>(16 * tn);
        dXo = A.out<float>(3 * tm);
    });
    if (rc) return rc;
    rc = orbgpu_optimize_essential_graph_device(n_kf, n_edges, n_points, dT, dhc, dSc, dhn, dSn, dfix, dei, dej, dkind,
                                                dX, dref, fix_scale, n_iterations, dSo, dTo, dXo, result, d_workspace,
                                                workspace_bytes, ctx->stream);
    if (rc) return rc;
    if (result->status == 0) {
        call.fetch(dSo, Scw_out, sizeof(double) * 8 * tn);
        call.fetch(dTo, Tcw_out, sizeof(float) * 16 * tn);
        call.fetch(dXo, Xw_out, sizeof(float) * 3 * tm);
    }
    return call.finish();
}
