// globalba.hip -- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt
// (src/Optimizer.cpp:72-269) for ONE problem spread over the whole chip
// (include/orbgpu_globalba.h): the arithmetic of localba.hip -- the two
// projection edges with their Jacobians, the quadratic form, the Schur
// complement onto the poses, g2o's Levenberg-Marquardt over the whole vector and
// the active set of initializeOptimization(0) -- as one launch per phase, and a
// dense blocked Cholesky of the reduced system that runs over all compute units
// (chol_blocked.h, shared with essential.hip).
// tests/globalba_ref.py is the same arithmetic, expression for expression.
// SE3Quat is se3_device.h's, the Huber thresholds are projection_edge.h's and
// the field offsets ba_schur_device.h's, shared with localba.hip; the control
// block, the host record, the ordered sums and the bodies of the begin and
// judge kernels are wholechip_lm.h's, shared with essential.hip; the pose
// write-out is lm_device.h's, the LM decisions are lm_runtime.h's.  The
// kernels are ba_phases.h's, instantiated here over Args (no levels);
// localba_chip.hip instantiates them with LocalBA's levels.  They keep their
// own bodies over Args: the per-item arithmetic is ba_schur_device.h's text,
// and moving the kernels onto its view measured 0.5-0.9 % slower in ba_schur
// (§5q found what changes that kernel's code).
//
// The calling thread drives the loop.  A phase that needs the previous one
// complete is the next launch on the stream; no kernel synchronises with
// another workgroup, spins on memory or is launched cooperatively.  A one-wave
// judge kernel advances lm::Run in the workspace and copies its decisions into a
// coherent pinned host record; the host synchronises the stream once per trial,
// reads the record, polls the stop flag where g2o polls it and enqueues the
// next trial or iteration: at most n_iterations (1 + 10) passes on any input.
//
// Every sum has one owner that adds its terms in a fixed order, and there are no
// floating-point atomics:
//   entry v of a pose's 21 + 6      one lane, over the pose's edges ascending (a pose-major edge
//                                   list built once per call by a ballot scan: exact in any order)
//   entry v of a point's 6 + 3      one lane, over the point's run of edges
//   entry (r, s) of block (a, b)    one lane (36 per block), over the pairs (e, e2) of
//     of the reduced system         localba_ref.structure's order: e over pose a's edges ascending,
//                                   e2 over the edges of e's point seen from pose b ascending.  The
//                                   pairs are found by a merge of the two poses' edge lists on the
//                                   point index (both ascend with the edge index), not read from
//                                   stored pair lists: their number is not bounded by the counts the
//                                   workspace is sized from
//   entry (i, j) of the factor      A(i, j) - sum_k L(i, k) L(j, k) in ascending k: panel by panel in
//                                   the trailing update, then inside its own panel; the bits do not
//                                   depend on kNB or the tiling and equal the unblocked loop's.
//                                   b_schur is row n of the matrix: its factor row is y
//   s[k] of the back-substitution   s[k] -= L(i, k) x[i] in descending i
//   robust chi2, computeScale       per-workgroup partial sums in index order (16 lanes add 16
//                                   values each, lane 0 the 16 sums), added in workgroup order by
//                                   lane 0 of the judge kernel
//   computeLambdaInit's maximum     integer atomicMax on the bits of |H_jj| (non-negative doubles
//                                   order as their bits; a NaN is the largest)
// A pivot that is not positive sets a word; every later kernel of that trial returns at once on it.
// Loop bounds are counts of the index structure, never floating-point values.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/orbgpu_globalba.h"
#include "ba_phases.h"
#include "chol_blocked.h"
#include "host_common.h"
#include "host_ctx.h"

namespace {

using namespace orbgpu::ba_phases;  // the kernels, their Args and Ctl, the field offsets

constexpr int kEdgeD = 67, kPointI = 2;  // doubles per edge, ints per point: ba_schur_device.h's fields alone

struct Layout {
    size_t P, M, E, n_max;                            // n_max = 6 P
    size_t pose_d, point_d, edge_d, sys_d, x_d, chi_d, scale_d;  // in doubles, after the control block
    size_t n_chi, n_scale;
    size_t ints;                                      // byte offset of the ints
    size_t pose_i, point_i, edge_i;
    size_t bytes;                                     // 0: does not fit
};

inline Layout make_layout(int n_poses, int n_points, int n_edges) {
    Layout l;
    std::memset(&l, 0, sizeof(l));
    typedef unsigned __int128 u128;
    const u128 P = (u128)n_poses, M = (u128)n_points, E = (u128)n_edges, n = 6 * P;
    const u128 n_chi = (E + kThreads - 1) / kThreads, n_scale = (P + M + kThreads - 1) / kThreads;
    const u128 doubles = kPoseD * P + kPointD * M + kEdgeD * E + (n + 1) * n + n + n_chi + n_scale;
    const u128 ints = kPoseI * P + kPointI * M + E;
    const u128 bytes = kCtlBytes + doubles * 8 + ((ints * 4 + 7) / 8) * 8 + 8;
    if (bytes > (u128)(SIZE_MAX / 2)) return l;
    l.P = (size_t)P, l.M = (size_t)M, l.E = (size_t)E, l.n_max = (size_t)n;
    l.n_chi = (size_t)n_chi, l.n_scale = (size_t)n_scale;
    l.pose_d = 0;
    l.point_d = l.pose_d + kPoseD * l.P;
    l.edge_d = l.point_d + kPointD * l.M;
    l.sys_d = l.edge_d + kEdgeD * l.E;
    l.x_d = l.sys_d + (l.n_max + 1) * l.n_max;
    l.chi_d = l.x_d + l.n_max;
    l.scale_d = l.chi_d + l.n_chi;
    l.ints = kCtlBytes + (size_t)doubles * 8;
    l.pose_i = 0;
    l.point_i = l.pose_i + kPoseI * l.P;
    l.edge_i = l.point_i + kPointI * l.M;
    l.bytes = (size_t)bytes;
    return l;
}

// what chol_blocked.h's kernels read of the workspace
struct SystemView {
    double *S, *x;
    int* fail;
    const int* nf;
    __device__ size_t n() const { return 6 * (size_t)*nf; }
};

// the kernels: ba_phases.h's, over Args (no levels)
constexpr auto k_check = ba_check<Args>;
constexpr auto k_init = ba_init<Args>;
constexpr auto k_runs = ba_runs<Args>;
constexpr auto k_scan = ba_scan<Args>;
constexpr auto k_lists = ba_lists<Args>;
constexpr auto k_edges_build = ba_edges<Args, true>;
constexpr auto k_edges_trial = ba_edges<Args, false>;
constexpr auto k_vertex_sums = ba_vertex_sums<Args>;
constexpr auto k_begin = ba_begin<Args>;
constexpr auto k_point_inverse = ba_point_inverse<Args>;
constexpr auto k_edge_bd = ba_edge_bd<Args>;
constexpr auto k_schur = ba_schur<Args>;
constexpr auto k_point_x = ba_point_x<Args>;
constexpr auto k_trial = ba_trial<Args>;
constexpr auto k_judge = ba_judge<Args>;
constexpr auto k_accept = ba_accept<Args>;
constexpr auto k_write = ba_write<Args>;

#undef PD
#undef LD
#undef ED
#undef PI
#undef LI

// ------------------------------------------------------------------ host

int check_args(int n_poses, int n_points, int n_edges, int n_iterations, bool pose_arrays, bool point_arrays,
               bool edge_arrays, bool result) {
    using orbgpu::fail;
    if (n_poses < 0 || n_points < 0 || n_edges < 0 || n_iterations < 0)
        return fail(ORBGPU_ERR_ARG, "negative count or n_iterations");
    if (!result) return fail(ORBGPU_ERR_ARG, "null result");
    if (n_poses > 0 && !pose_arrays) return fail(ORBGPU_ERR_ARG, "null pose array");
    if (n_points > 0 && !point_arrays) return fail(ORBGPU_ERR_ARG, "null point array");
    if (n_edges > 0 && !edge_arrays) return fail(ORBGPU_ERR_ARG, "null edge array");
    return ORBGPU_OK;
}

inline bool flag_set(const volatile uint8_t* stop_flag) { return stop_flag && *stop_flag; }

}  // namespace

extern "C" size_t orbgpu_bundle_adjustment_workspace_bytes(int n_poses, int n_points, int n_edges) {
    if (n_poses < 0 || n_points < 0 || n_edges < 0) return 0;
    return make_layout(n_poses, n_points, n_edges).bytes;
}

extern "C" int orbgpu_bundle_adjustment_device(int n_poses, int n_points, int n_edges, const float* d_Tcw,
                                               const uint8_t* d_fixed, const float* d_cam, const float* d_Xw,
                                               const int* d_edge_pose, const int* d_edge_point, const float* d_obs,
                                               const float* d_inv_sigma2, int n_iterations, int robust,
                                               const volatile uint8_t* stop_flag, float* d_Tcw_out, float* d_Xw_out,
                                               orbgpu_ba_result* result, void* d_workspace, size_t workspace_bytes,
                                               void* stream) {
    if (int rc = check_args(n_poses, n_points, n_edges, n_iterations, d_Tcw && d_fixed && d_cam && d_Tcw_out,
                            d_Xw && d_Xw_out, d_edge_pose && d_edge_point && d_obs && d_inv_sigma2, result))
        return rc;
    const Layout L = make_layout(n_poses, n_points, n_edges);
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
    a.P = n_poses, a.M = n_points, a.E = n_edges, a.robust = robust ? 1 : 0;
    a.Tcw = d_Tcw, a.cam = d_cam, a.Xw = d_Xw, a.obs = d_obs, a.inv_sigma2 = d_inv_sigma2, a.fixed = d_fixed;
    a.edge_pose = d_edge_pose, a.edge_point = d_edge_point, a.Tcw_out = d_Tcw_out, a.Xw_out = d_Xw_out;
    uint8_t* base = static_cast<uint8_t*>(d_workspace);
    a.ctl = reinterpret_cast<Ctl*>(base);
    a.rec = rec;
    double* d = reinterpret_cast<double*>(base + kCtlBytes);
    a.wp = d + L.pose_d, a.wl = d + L.point_d, a.we = d + L.edge_d, a.S = d + L.sys_d, a.x = d + L.x_d;
    a.chi_part = d + L.chi_d, a.scale_part = d + L.scale_d;
    int* ints = reinterpret_cast<int*>(base + L.ints);
    a.ip = ints + L.pose_i, a.il = ints + L.point_i, a.ie = ints + L.edge_i;
    a.n_chi = (int)L.n_chi, a.n_scale = (int)L.n_scale;
    const auto hc = orbgpu::proj_edge::huber_constants(5.99, 7.815);  // Optimizer.cpp:112-113
    a.delta_mono = hc.delta_mono, a.delta_stereo = hc.delta_stereo;
    a.dsqr_mono = hc.dsqr_mono, a.dsqr_stereo = hc.dsqr_stereo;

    SystemView view;
    view.S = a.S, view.x = a.x, view.fail = &a.ctl->fail, view.nf = &a.ctl->nf;

    const size_t P = L.P, M = L.M, E = L.E;
    const dim3 T(kThreads);
    // once per call: the check, the estimates and the structure; one synchronisation
    ORB_HIP(hipMemsetAsync(a.ctl, 0, kCtlBytes, st));
    if (E) ORB_LAUNCH(st, k_check, dim3(blocks_for(E)), T, a);
    if (P + M) ORB_LAUNCH(st, k_init, dim3(blocks_for(P > M ? P : M)), T, a);
    if (E) ORB_LAUNCH(st, k_runs, dim3(blocks_for(E)), T, a);
    ORB_LAUNCH(st, k_scan, dim3(1), dim3(64), a);
    if (E && P) ORB_LAUNCH(st, k_lists, dim3(blocks_for(P, kThreads / 64)), T, a);
    ORB_HIP(hipStreamSynchronize(st));
    if (rec->bad) {
        result->status = -1;
        return ORBGPU_OK;
    }
    const int nf = rec->nf;
    const size_t n = 6 * (size_t)nf;
    result->n_free = nf, result->n_active_points = rec->n_active;

    int stopped = 0, iterations = 0;
    bool done = false;
    if (nf + rec->n_active > 0) {  // optimize() returns at once without an active vertex
        for (int it = 0; it < n_iterations; ++it) {
            if (flag_set(stop_flag)) {  // sparse_optimizer.cpp:376
                stopped = 1;
                break;
            }
            if (done) break;
            ORB_LAUNCH(st, k_edges_build, dim3(blocks_for(E)), T, a);
            ORB_LAUNCH(st, k_vertex_sums, dim3(blocks_for(P * 27 + M * 9)), T, a, it == 0 ? 1 : 0);
            ORB_LAUNCH(st, k_begin, dim3(1), dim3(64), a, it == 0 ? 1 : 0);
            iterations = it + 1;
            for (int trial = 0; trial < lm::kMaxTrials; ++trial) {
                ORB_LAUNCH(st, k_point_inverse, dim3(blocks_for(M)), T, a);
                ORB_LAUNCH(st, k_edge_bd, dim3(blocks_for(E)), T, a);
                if (nf) {
                    ORB_LAUNCH(st, k_schur, dim3(blocks_for((size_t)nf * nf * 36 + n)), T, a);
                    ORB_HIP(orbgpu::chol::enqueue_solve(view, n, st));
                }
                ORB_LAUNCH(st, k_point_x, dim3(blocks_for(M)), T, a);
                ORB_LAUNCH(st, k_trial, dim3(blocks_for(P + M)), T, a);
                ORB_LAUNCH(st, k_edges_trial, dim3(blocks_for(E)), T, a);
                ORB_LAUNCH(st, k_judge, dim3(1), dim3(64), a, n_iterations);
                ORB_HIP(hipStreamSynchronize(st));
                if (rec->accepted) ORB_LAUNCH(st, k_accept, dim3(blocks_for(P * 7 > M * 3 ? P * 7 : M * 3)), T, a);
                if (!rec->more) break;
                if (flag_set(stop_flag)) {  // optimization_algorithm_levenberg.cpp:149
                    stopped = 2;
                    break;
                }
            }
            if (stopped) break;
            // run_end_iteration also ends at iter >= n_iterations: the loop's own bound
            done = rec->done != 0;
        }
    }
    if (P + M) ORB_LAUNCH(st, k_write, dim3(blocks_for(P > M ? P : M)), T, a);
    ORB_HIP(hipStreamSynchronize(st));
    result->iterations = iterations;
    result->rejected = rec->rejected;
    result->stopped = stopped;
    result->iterations_applied = stopped == 2 ? iterations - 1 : iterations;
    result->first_chi2 = rec->first_chi, result->last_chi2 = rec->chi, result->last_lambda = rec->lambda;
    return ORBGPU_OK;
}

extern "C" int orbgpu_bundle_adjustment(int n_poses, int n_points, int n_edges, const float* Tcw, const uint8_t* fixed,
                                        const float* cam, const float* Xw, const int* edge_pose, const int* edge_point,
                                        const float* obs, const float* inv_sigma2, int n_iterations, int robust,
                                        const volatile uint8_t* stop_flag, float* Tcw_out, float* Xw_out,
                                        orbgpu_ba_result* result, void* d_workspace, size_t workspace_bytes) {
    using namespace orbgpu;
    int rc = check_args(n_poses, n_points, n_edges, n_iterations, Tcw && fixed && cam && Tcw_out, Xw && Xw_out,
                        edge_pose && edge_point && obs && inv_sigma2, result);
    if (rc) return rc;
    for (int i = 0; i < n_edges; ++i) {
        const int p = edge_pose[i], m = edge_point[i];
        if (p < 0 || p >= n_poses || m < 0 || m >= n_points)
            return fail(ORBGPU_ERR_ARG, "edge " + std::to_string(i) + ": an index is out of range");
        if (i > 0 && edge_point[i - 1] > m) return fail(ORBGPU_ERR_ARG, "edge " + std::to_string(i) + ": point indices decrease");
    }
    const size_t need = orbgpu_bundle_adjustment_workspace_bytes(n_poses, n_points, n_edges);
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
    const size_t tp = (size_t)n_poses, tm = (size_t)n_points, te = (size_t)n_edges;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    HostCall call(*ctx);
    const float *dT, *dcam, *dX, *dobs, *dw;
    const uint8_t* dfix;
    const int *dep, *del;
    float *dTo, *dXo;
    rc = call.run([&](HostCall& A) {
        dT = A.in(Tcw, 12 * tp);
        dfix = A.in(fixed, tp);
        dcam = A.in(cam, 5 * tp);
        dX = A.in(Xw, 3 * tm);
        dep = A.in(edge_pose, te);
        del = A.in(edge_point, te);
        dobs = A.in(obs, 3 * te);
        dw = A.in(inv_sigma2, te);
        dTo = A.out<float>(16 * tp);
        dXo = A.out<float>(3 * tm);
    });
    if (rc) return rc;
    rc = orbgpu_bundle_adjustment_device(n_poses, n_points, n_edges, dT, dfix, dcam, dX, dep, del, dobs, dw,
                                         n_iterations, robust, stop_flag, dTo, dXo, result, d_workspace,
                                         workspace_bytes, ctx->stream);
    if (rc) return rc;
    call.fetch(dTo, Tcw_out, sizeof(float) * 16 * tp);
    call.fetch(dXo, Xw_out, sizeof(float) * 3 * tm);
    return call.finish();
}
