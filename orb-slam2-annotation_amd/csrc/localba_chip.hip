// localba_chip.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:
// 536-885) of ONE neighbourhood spread over the whole chip
// (include/orbgpu_localba_chip.h): LocalBA's two rounds, level-1 edges and
// erase flags (localba.hip keeps them inside one workgroup) on the phases of
// globalba.hip, a launch each, with g2o's polls of the stop flag made by the
// host loop.  tests/localba_chip_ref.py is the same arithmetic, expression
// for expression.
//
// The phases are ba_phases.h's, instantiated over LevelArgs: a level word per
// edge masks the edge in the build and trial passes, in the vertex sums and in
// the merge of the Schur assembly, and one more double per edge keeps the chi2
// of the last pass that evaluated it.  What this file adds on the device:
//   chip_classify   one lane per edge: chi2 > 5.991 | 7.815 || !(z > 0) at the kept
//                   estimates, into the level words (after the first round) or the
//                   erase bytes (at the end); the count by a ballot and one integer
//                   atomic per wave
//   chip_active     the second round's active set: a wave per pose walks the pose's
//                   list for a level-0 edge (IP_FREE), a lane per point walks the
//                   point's run and empties it when none is left; ba_scan then
//                   numbers the free poses (hidx may get gaps, n_free may shrink)
// The rules are globalba.hip's: fp64 under -ffp-contract=off, no
// floating-point atomics, every sum has one owner that adds in a fixed order,
// no synchronisation between workgroups inside a launch, loop bounds are counts
// of the index structure.  One exception to "every later kernel of a failed
// trial returns at once": the trial edge pass runs after a failed solve, on the
// kept estimates (ba_phases.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/orbgpu_localba_chip.h"
#include "ba_phases.h"
#include "chol_blocked.h"
#include "host_common.h"
#include "host_ctx.h"

namespace {

using namespace orbgpu::ba_phases;

constexpr int kEdgeD = 67 + 1, kPointI = 2;  // ba_schur_device.h's fields and the last chi2; a point's run
constexpr int kEdgeI = 2;                    // the pose-major list and the level word
constexpr size_t kCountBytes = 64;           // LevelArgs::counts, after the control block
constexpr double kThMono = 5.991, kThStereo = 7.815;  // Optimizer.cpp:782, 798

struct Layout {
    size_t P, NL, M, E, n_max;                                   // n_max = 6 NL
    size_t pose_d, point_d, edge_d, sys_d, x_d, chi_d, scale_d;  // in doubles, after the control block and the counts
    size_t n_chi, n_scale;
    size_t ints;                                                 // byte offset of the ints
    size_t pose_i, point_i, edge_i;
    size_t bytes;                                                // 0: does not fit
};

inline Layout make_layout(int n_poses, int n_local, int n_points, int n_edges) {
    Layout l;
    std::memset(&l, 0, sizeof(l));
    typedef unsigned __int128 u128;
    const u128 P = (u128)n_poses, M = (u128)n_points, E = (u128)n_edges, n = 6 * (u128)n_local;
    const u128 n_chi = (E + kThreads - 1) / kThreads, n_scale = (P + M + kThreads - 1) / kThreads;
    const u128 doubles = kPoseD * P + kPointD * M + kEdgeD * E + (n + 1) * n + n + n_chi + n_scale;
    const u128 ints = kPoseI * P + kPointI * M + kEdgeI * E;
    const u128 bytes = kCtlBytes + kCountBytes + doubles * 8 + ((ints * 4 + 7) / 8) * 8 + 8;
    if (bytes > (u128)(SIZE_MAX / 2)) return l;
    l.P = (size_t)P, l.NL = (size_t)n_local, l.M = (size_t)M, l.E = (size_t)E, l.n_max = (size_t)n;
    l.n_chi = (size_t)n_chi, l.n_scale = (size_t)n_scale;
    l.pose_d = 0;
    l.point_d = l.pose_d + kPoseD * l.P;
    l.edge_d = l.point_d + kPointD * l.M;
    l.sys_d = l.edge_d + kEdgeD * l.E;
    l.x_d = l.sys_d + (l.n_max + 1) * l.n_max;
    l.chi_d = l.x_d + l.n_max;
    l.scale_d = l.chi_d + l.n_chi;
    l.ints = kCtlBytes + kCountBytes + (size_t)doubles * 8;
    l.pose_i = 0;
    l.point_i = l.pose_i + kPoseI * l.P;
    l.edge_i = l.point_i + kPointI * l.M;
    l.bytes = (size_t)bytes;
    return l;
}

// ------------------------------------------------------------------ what the levels add on the device

// the test of :779-803 and :823-847 at the kept estimates, one lane per edge
__global__ __launch_bounds__(kThreads) void chip_classify(LevelArgs A, int final_test) {
    const size_t gi = global_tid();
    bool flag = false;
    if (gi < (size_t)A.E) {
        const int i = (int)gi;
        double x, y, z, e[3], q[4], w;
        bool stereo;
        const float* cam;
        (void)edge_error(A, i, P_EST, L_EST, x, y, z, e, q, w, stereo, cam);
        flag = A.last_chi2[i] > (stereo ? kThStereo : kThMono) || !(z > 0.0);
        if (final_test)
            A.erase[i] = flag ? 1 : 0;
        else
            A.level[i] = flag ? 1 : 0;
    }
    const unsigned long long mask = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&A.counts[final_test ? 1 : 0], (int)__popcll(mask));
}

// initializeOptimization(0) after the classification: the first pose_blocks workgroups take a pose
// per wave, the others a point per lane
__global__ __launch_bounds__(kThreads) void chip_active(LevelArgs A, int pose_blocks) {
    if ((int)blockIdx.x < pose_blocks) {
        const int lane = threadIdx.x & 63;
        const int p = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
        if (p >= A.P) return;  // a whole wave
        const int start = PI(IP_START, p), count = PI(IP_COUNT, p);
        bool any = false;
        for (int s0 = 0; s0 < count; s0 += 64) {
            const int s = s0 + lane;
            const bool active = s < count && A.level[A.ie[start + s]] == 0;
            any = any || __ballot(active) != 0;
        }
        if (lane == 0) PI(IP_FREE, p) = any && !pose_fixed(A, p);
        return;
    }
    const size_t gi = (size_t)(blockIdx.x - pose_blocks) * kThreads + threadIdx.x;
    if (gi >= (size_t)A.M) return;
    const int m = (int)gi;
    const int begin = LI(IL_FIRST, m), end = LI(IL_END, m);
    if (end <= begin) return;
    bool any = false;
    for (int e = begin; e < end; ++e) any = any || A.level[e] == 0;
    if (any)
        atomicAdd(&A.counts[2], 1);
    else
        LI(IL_END, m) = begin;  // an empty run: the point is not optimised, not damped, not in the maximum
}

#undef PD
#undef LD
#undef ED
#undef PI
#undef LI

// what chol_blocked.h's kernels read of the workspace
struct SystemView {
    double *S, *x;
    int* fail;
    const int* nf;
    __device__ size_t n() const { return 6 * (size_t)*nf; }
};

constexpr auto k_check = ba_check<LevelArgs>;
constexpr auto k_init = ba_init<LevelArgs>;
constexpr auto k_runs = ba_runs<LevelArgs>;
constexpr auto k_scan = ba_scan<LevelArgs>;
constexpr auto k_lists = ba_lists<LevelArgs>;
constexpr auto k_edges_build = ba_edges<LevelArgs, true>;
constexpr auto k_edges_trial = ba_edges<LevelArgs, false>;
constexpr auto k_vertex_sums = ba_vertex_sums<LevelArgs>;
constexpr auto k_begin = ba_begin<LevelArgs>;
constexpr auto k_point_inverse = ba_point_inverse<LevelArgs>;
constexpr auto k_edge_bd = ba_edge_bd<LevelArgs>;
constexpr auto k_schur = ba_schur<LevelArgs>;
constexpr auto k_point_x = ba_point_x<LevelArgs>;
constexpr auto k_trial = ba_trial<LevelArgs>;
constexpr auto k_judge = ba_judge<LevelArgs>;
constexpr auto k_accept = ba_accept<LevelArgs>;
constexpr auto k_write = ba_write<LevelArgs>;

// ------------------------------------------------------------------ host

// the force-stop flag as g2o's terminate() reads it, and the replay of a recorded poll
struct Polls {
    const volatile uint8_t* flag;
    int stop_at;
    orbgpu_localba_chip_result* res;
    bool operator()() const {
        const int k = res->polls++;
        const bool seen = (stop_at >= 0 && k >= stop_at) || (flag && *flag);
        if (seen && res->stop_poll < 0) res->stop_poll = k;
        return seen;
    }
};

// SparseOptimizer::optimize(n_iterations) over round r's active set: globalba.hip's loop
int run_round(const LevelArgs& a, const SystemView& view, const Layout& L, HostRec* rec, int n_iterations, int r,
              const Polls& poll, hipStream_t st) {
    orbgpu_localba_chip_result* res = poll.res;
    const int nf = rec->nf;
    if (nf + rec->n_active == 0) return ORBGPU_OK;  // optimize() returns at once without an active vertex
    const size_t n = 6 * (size_t)nf, P = L.P, M = L.M, E = L.E;
    const dim3 T(kThreads);
    int stopped = 0, iterations = 0, rejected = 0;
    bool done = false;
    for (int it = 0; it < n_iterations; ++it) {
        if (poll()) {  // sparse_optimizer.cpp:376
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
            rejected = rec->rejected;
            if (rec->accepted) ORB_LAUNCH(st, k_accept, dim3(blocks_for(P * 7 > M * 3 ? P * 7 : M * 3)), T, a);
            if (!rec->more) break;
            if (poll()) {  // optimization_algorithm_levenberg.cpp:149
                stopped = 2;
                break;
            }
        }
        if (stopped) break;
        done = rec->done != 0;
    }
    res->lm_iterations[r] = iterations, res->lm_rejected[r] = rejected, res->stopped[r] = stopped;
    res->iterations_applied[r] = stopped == 2 ? iterations - 1 : iterations;
    return ORBGPU_OK;
}

int check_args(int n_poses, int n_local, int n_points, int n_edges, int iterations_first, int iterations_second,
               int stop_at_poll, bool pose_arrays, bool local_arrays, bool point_arrays, bool edge_arrays, bool result) {
    using orbgpu::fail;
    if (n_poses < 0 || n_local < 0 || n_points < 0 || n_edges < 0 || iterations_first < 0 || iterations_second < 0)
        return fail(ORBGPU_ERR_ARG, "negative count or iteration number");
    if (n_local > n_poses) return fail(ORBGPU_ERR_ARG, "n_local > n_poses");
    if (stop_at_poll < -1) return fail(ORBGPU_ERR_ARG, "stop_at_poll < -1");
    if (!result) return fail(ORBGPU_ERR_ARG, "null result");
    if (n_poses > 0 && !pose_arrays) return fail(ORBGPU_ERR_ARG, "null pose array");
    if (n_local > 0 && !local_arrays) return fail(ORBGPU_ERR_ARG, "null pose output array");
    if (n_points > 0 && !point_arrays) return fail(ORBGPU_ERR_ARG, "null point array");
    if (n_edges > 0 && !edge_arrays) return fail(ORBGPU_ERR_ARG, "null edge array");
    return ORBGPU_OK;
}

}  // namespace

extern "C" size_t orbgpu_local_ba_chip_workspace_bytes(int n_poses, int n_local, int n_points, int n_edges) {
    if (n_poses < 0 || n_local < 0 || n_points < 0 || n_edges < 0 || n_local > n_poses) return 0;
    return make_layout(n_poses, n_local, n_points, n_edges).bytes;
}

extern "C" int orbgpu_local_ba_chip_device(int n_poses, int n_local, int n_points, int n_edges, const float* d_Tcw,
                                           const uint8_t* d_fixed, const float* d_cam, const float* d_Xw,
                                           const int* d_edge_pose, const int* d_edge_point, const float* d_obs,
                                           const float* d_inv_sigma2, int iterations_first, int iterations_second,
                                           const volatile uint8_t* stop_flag, int stop_at_poll, float* d_Tcw_out,
                                           float* d_Xw_out, uint8_t* d_erase, orbgpu_localba_chip_result* result,
                                           void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_args(n_poses, n_local, n_points, n_edges, iterations_first, iterations_second, stop_at_poll,
                            d_Tcw && d_fixed && d_cam, d_Tcw_out, d_Xw && d_Xw_out,
                            d_edge_pose && d_edge_point && d_obs && d_inv_sigma2 && d_erase, result))
        return rc;
    const Layout L = make_layout(n_poses, n_local, n_points, n_edges);
    if (!d_workspace || ((uintptr_t)d_workspace & 7) || L.bytes == 0 || workspace_bytes < L.bytes)
        return orbgpu::fail(ORBGPU_ERR_ARG, "null, misaligned or too small workspace, or a size that does not fit");
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    std::memset(result, 0, sizeof(*result));
    result->stop_poll = -1;
    HostRec* rec;
    if (int rc = wc::host_rec(&rec)) return rc;
    std::memset(rec, 0, sizeof(*rec));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    LevelArgs a;
    a.P = n_poses, a.M = n_points, a.E = n_edges, a.robust = 1;
    a.Tcw = d_Tcw, a.cam = d_cam, a.Xw = d_Xw, a.obs = d_obs, a.inv_sigma2 = d_inv_sigma2, a.fixed = d_fixed;
    a.edge_pose = d_edge_pose, a.edge_point = d_edge_point, a.Tcw_out = d_Tcw_out, a.Xw_out = d_Xw_out;
    uint8_t* base = static_cast<uint8_t*>(d_workspace);
    a.ctl = reinterpret_cast<Ctl*>(base);
    a.counts = reinterpret_cast<int*>(base + kCtlBytes);
    a.rec = rec;
    double* d = reinterpret_cast<double*>(base + kCtlBytes + kCountBytes);
    a.wp = d + L.pose_d, a.wl = d + L.point_d, a.we = d + L.edge_d, a.S = d + L.sys_d, a.x = d + L.x_d;
    a.last_chi2 = a.we + (size_t)(kEdgeD - 1) * L.E;
    a.chi_part = d + L.chi_d, a.scale_part = d + L.scale_d;
    int* ints = reinterpret_cast<int*>(base + L.ints);
    a.ip = ints + L.pose_i, a.il = ints + L.point_i, a.ie = ints + L.edge_i, a.level = a.ie + L.E;
    a.n_chi = (int)L.n_chi, a.n_scale = (int)L.n_scale;
    a.n_local = n_local, a.second_round = 0, a.erase = d_erase;
    const auto hc = orbgpu::proj_edge::huber_constants(kThMono, kThStereo);  // Optimizer.cpp:666-667
    a.delta_mono = hc.delta_mono, a.delta_stereo = hc.delta_stereo;
    a.dsqr_mono = hc.dsqr_mono, a.dsqr_stereo = hc.dsqr_stereo;

    SystemView view;
    view.S = a.S, view.x = a.x, view.fail = &a.ctl->fail, view.nf = &a.ctl->nf;

    const size_t P = L.P, M = L.M, E = L.E;
    const dim3 T(kThreads);
    const Polls poll{stop_flag, stop_at_poll, result};
    int counts[3] = {0, 0, 0};
    // once per call: the check, the estimates and the structure; one synchronisation
    ORB_HIP(hipMemsetAsync(base, 0, kCtlBytes + kCountBytes, st));
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
    if (E) {
        result->n_free[0] = rec->nf, result->n_active_points[0] = rec->n_active;
        if (int rc = run_round(a, view, L, rec, iterations_first, 0, poll, st)) return rc;
        result->rounds = 1;
        if (!poll()) {  // Optimizer.cpp:764-766: a read of its own
            const unsigned pose_blocks = blocks_for(P, kThreads / 64);
            ORB_LAUNCH(st, chip_classify, dim3(blocks_for(E)), T, a, 0);
            ORB_LAUNCH(st, chip_active, dim3(pose_blocks + blocks_for(M)), T, a, (int)pose_blocks);
            a.second_round = 1, a.robust = 0;
            ORB_LAUNCH(st, k_scan, dim3(1), dim3(64), a);
            ORB_HIP(hipMemcpyAsync(counts, a.counts, sizeof(counts), hipMemcpyDeviceToHost, st));
            ORB_HIP(hipStreamSynchronize(st));  // the second round's active set
            result->n_bad_first = counts[0];
            result->n_free[1] = rec->nf, result->n_active_points[1] = rec->n_active;
            if (int rc = run_round(a, view, L, rec, iterations_second, 1, poll, st)) return rc;
            result->rounds = 2;
        }
        ORB_LAUNCH(st, chip_classify, dim3(blocks_for(E)), T, a, 1);
    }
    if (P + M) ORB_LAUNCH(st, k_write, dim3(blocks_for(P > M ? P : M)), T, a);
    ORB_HIP(hipMemcpyAsync(counts, a.counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    ORB_HIP(hipStreamSynchronize(st));
    result->n_erase = counts[1];
    return ORBGPU_OK;
}

extern "C" int orbgpu_local_ba_chip(int n_poses, int n_local, int n_points, int n_edges, const float* Tcw,
                                    const uint8_t* fixed, const float* cam, const float* Xw, const int* edge_pose,
                                    const int* edge_point, const float* obs, const float* inv_sigma2,
                                    int iterations_first, int iterations_second, const volatile uint8_t* stop_flag,
                                    int stop_at_poll, float* Tcw_out, float* Xw_out, uint8_t* erase,
                                    orbgpu_localba_chip_result* result, void* d_workspace, size_t workspace_bytes) {
    using namespace orbgpu;
    int rc = check_args(n_poses, n_local, n_points, n_edges, iterations_first, iterations_second, stop_at_poll,
                        Tcw && fixed && cam, Tcw_out, Xw && Xw_out, edge_pose && edge_point && obs && inv_sigma2 && erase,
                        result);
    if (rc) return rc;
    for (int i = 0; i < n_edges; ++i) {
        const int p = edge_pose[i], m = edge_point[i];
        if (p < 0 || p >= n_poses || m < 0 || m >= n_points)
            return fail(ORBGPU_ERR_ARG, "edge " + std::to_string(i) + ": an index is out of range");
        if (i > 0 && edge_point[i - 1] > m) return fail(ORBGPU_ERR_ARG, "edge " + std::to_string(i) + ": point indices decrease");
    }
    const size_t need = orbgpu_local_ba_chip_workspace_bytes(n_poses, n_local, n_points, n_edges);
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
    const size_t tp = (size_t)n_poses, tl = (size_t)n_local, tm = (size_t)n_points, te = (size_t)n_edges;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    HostCall call(*ctx);
    const float *dT, *dcam, *dX, *dobs, *dw;
    const uint8_t* dfix;
    const int *dep, *del;
    float *dTo, *dXo;
    uint8_t* der;
    rc = call.run([&](HostCall& A) {
        dT = A.in(Tcw, 12 * tp);
        dfix = A.in(fixed, tp);
        dcam = A.in(cam, 5 * tp);
        dX = A.in(Xw, 3 * tm);
        dep = A.in(edge_pose, te);
        del = A.in(edge_point, te);
        dobs = A.in(obs, 3 * te);
        dw = A.in(inv_sigma2, te);
        dTo = A.out<float>(16 * tl);
        dXo = A.out<float>(3 * tm);
        der = A.out<uint8_t>(te);
    });
    if (rc) return rc;
    rc = orbgpu_local_ba_chip_device(n_poses, n_local, n_points, n_edges, dT, dfix, dcam, dX, dep, del, dobs, dw,
                                     iterations_first, iterations_second, stop_flag, stop_at_poll, dTo, dXo, der,
                                     result, d_workspace, workspace_bytes, ctx->stream);
    if (rc) return rc;
    call.fetch(dTo, Tcw_out, sizeof(float) * 16 * tl);
    call.fetch(dXo, Xw_out, sizeof(float) * 3 * tm);
    call.fetch(der, erase, te);
    return call.finish();
}
