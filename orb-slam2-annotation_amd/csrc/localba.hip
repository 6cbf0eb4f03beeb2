// localba.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:536-885,
// the optimisation :759-847) for a batch of keyframe neighbourhoods
// (include/orbgpu_localba.h): the two binary projection edges with their
// analytic Jacobians (types/types_six_dof_expmap.cpp:112-168, 199-245), the
// quadratic form of a binary edge (core/base_binary_edge.hpp:43-120), the
// Schur complement onto the pose block, its dense solve and the
// back-substitution (core/block_solver.hpp:355-487, 565-610), g2o's
// Levenberg-Marquardt over the whole vector and the active set of
// initializeOptimization(0).  tests/localba_ref.py is the same arithmetic,
// expression for expression.  The arithmetic of one edge, pose or point -- the
// edges, the vertex blocks, Dinv, B Dinv, b_schur, the back-substitution, oplus
// -- and the workspace's field offsets are ba_schur_device.h's (over
// projection_edge.h and se3_device.h), shared with globalba.hip; Huber, the
// quaternion algebra and the pose write-out are lm_device.h's, the LM decisions
// lm_runtime.h's, the lane-order sum wholechip_lm.h's.  This file keeps the
// structure build, the assembly of S by half-row owners, the in-kernel column
// Cholesky, computeLambdaInit's maximum and the two rounds with their flagging.
//
// One workgroup per job, one launch for the whole call, no synchronisation
// between workgroups.  Everything a job keeps lives in its slice of the
// caller's workspace (structure of arrays, a job's edges, points and poses at
// its own offsets): the estimates and the trial, per edge the two Jacobians,
// the robust weight, the pose-point block B and B Dinv, per vertex its
// diagonal block and right-hand side, and the reduced system of (6 free
// poses)^2 doubles.  Every sum has one owner that walks its terms in a fixed
// order: entry v of a pose's block is summed by one lane over that pose's
// edges ascending (a pose-major edge list built once by the kernel), entry v
// of a point's block over the point's run of edges, half a row of the reduced
// system (three columns of every block) over the edges of the row's pose
// ascending and, inside, the run of the edge's point; the robust chi2 and computeScale's sum are per-lane
// strided partial sums added in lane order.  No floating-point atomics: a job's
// bytes do not depend on its neighbours, its block index or the call.
//
// Every loop is bounded by the reference's bounds, 5 (1 + 10) passes over the
// edges in the first round and 10 (1 + 10) in the second, and every branch
// around a barrier is taken on a word that one lane left in LDS before the
// barrier: the kernel ends on any input.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/orbgpu_localba.h"
#include "host_common.h"
#include "host_ctx.h"
#include "ba_schur_device.h"
#include "lm_runtime.h"
#include "wholechip_lm.h"

namespace {

namespace lm = orbgpu::lm;
namespace ba = orbgpu::ba;
using namespace orbgpu::ba;  // the field offsets
using orbgpu::proj_edge::HuberConst;

constexpr int kThreads = 256;
constexpr int kIterations[2] = {5, 10};  // optimizer.optimize(5), optimize(10): Optimizer.cpp:760, 809

// this file's fields beside ba_schur_device.h's: an edge's chi2 as the edge holds it, whether a point
// is active, and per edge its entry of the pose-major list and its level
constexpr int E_CHI = 67, kEdgeD = 68;
constexpr int kSysVecs = 5;  // column residues, diagonal of L, running sums, y, x
constexpr int IL_ACTIVE = 2, kPointI = 3;
constexpr int IE_LIST = 0, IE_LEVEL = 1, kEdgeI = 2;

struct Layout {
    size_t TP, TM, TE, n;                    // totals; n = 6 max_local
    size_t pose_d, point_d, edge_d, sys_d;   // in doubles
    size_t pose_i, point_i, edge_i;          // in ints, after the doubles
    size_t bytes;
};

__host__ __device__ inline Layout make_layout(int batch, int total_poses, int total_points, int total_edges,
                                              int max_local) {
    Layout l;
    l.TP = (size_t)total_poses, l.TM = (size_t)total_points, l.TE = (size_t)total_edges;
    l.n = 6 * (size_t)max_local;
    l.pose_d = 0;
    l.point_d = l.pose_d + kPoseD * l.TP;
    l.edge_d = l.point_d + kPointD * l.TM;
    l.sys_d = l.edge_d + kEdgeD * l.TE;
    const size_t doubles = l.sys_d + (size_t)batch * (l.n * l.n + kSysVecs * l.n);
    l.pose_i = 0;
    l.point_i = l.pose_i + kPoseI * l.TP;
    l.edge_i = l.point_i + kPointI * l.TM;
    const size_t ints = l.edge_i + kEdgeI * l.TE;
    l.bytes = doubles * sizeof(double) + ((ints * sizeof(int) + 7) & ~size_t(7)) + 8;
    return l;
}

struct Args {
    const orbgpu_localba_job* jobs;
    int batch, total_poses, total_local, total_points, total_edges, max_local;
    const float *Tcw, *cam, *Xw, *obs, *inv_sigma2;
    const uint8_t* fixed;
    const int *edge_pose, *edge_point;
    float *Tcw_out, *Xw_out;
    uint8_t* erase;
    orbgpu_localba_result* results;
    double* ws;
    HuberConst hc;
};

// every condition on a job's counts and ranges; host and device
__host__ __device__ inline bool job_ranges_ok(const orbgpu_localba_job& j, int total_poses, int total_local,
                                              int total_points, int total_edges, int max_local) {
    if (j.n_poses < 0 || j.n_local < 0 || j.n_points < 0 || j.n_edges < 0) return false;
    if (j.pose_offset < 0 || j.point_offset < 0 || j.edge_offset < 0 || j.out_pose_offset < 0) return false;
    if (j.n_local > j.n_poses || j.n_local > max_local) return false;
    return (long long)j.pose_offset + j.n_poses <= total_poses &&
           (long long)j.out_pose_offset + j.n_local <= total_local &&
           (long long)j.point_offset + j.n_points <= total_points &&
           (long long)j.edge_offset + j.n_edges <= total_edges;
}

// the job's state in LDS; written by lane 0 between barriers, read by all
struct Ctl {
    lm::Run run;
    double total;
    int valid, bad_index, P, NL, M, E, po, lo, eo, oo;
    int nf, n_active, solved, accepted, more, done, n_flag;
};

// wholechip::block_total, its total broadcast to every lane through c.total
__device__ inline double job_total(double v, double (&s_val)[kThreads], double (&s_row)[16], Ctl& c) {
    const double s = orbgpu::wholechip::block_total(v, s_val, s_row);
    if (threadIdx.x == 0) c.total = s;
    __syncthreads();
    return c.total;
}

__global__ __launch_bounds__(kThreads) void localba_kernel(Args A) {
    __shared__ Ctl c;
    __shared__ double s_val[kThreads];
    __shared__ double s_row[16];
    constexpr int T = kThreads;
    const int tid = threadIdx.x;
    const int jb = blockIdx.x;

    if (tid == 0) {
        const orbgpu_localba_job j = A.jobs[jb];
        c.valid = job_ranges_ok(j, A.total_poses, A.total_local, A.total_points, A.total_edges, A.max_local) ? 1 : 0;
        c.bad_index = 0;
        c.P = j.n_poses, c.NL = j.n_local, c.M = j.n_points, c.E = j.n_edges;
        c.po = j.pose_offset, c.lo = j.point_offset, c.eo = j.edge_offset, c.oo = j.out_pose_offset;
        c.n_flag = 0;
    }
    __syncthreads();
    orbgpu_localba_result* res = A.results + jb;
    if (!c.valid) {
        if (tid == 0) {
            res->rounds = -1, res->n_bad_first = 0, res->n_erase = 0, res->pad = 0;
            for (int k = 0; k < 2; ++k) res->lm_iterations[k] = 0, res->lm_rejected[k] = 0;
        }
        return;
    }
    const int P = c.P, NL = c.NL, M = c.M, E = c.E;
    const size_t po = (size_t)c.po, lo = (size_t)c.lo, eo = (size_t)c.eo;
    const int* epose = A.edge_pose + eo;
    const int* epoint = A.edge_point + eo;
    for (int i = tid; i < E; i += T) {
        const int p = epose[i], m = epoint[i];
        if (p < 0 || p >= P || m < 0 || m >= M || (i > 0 && epoint[i - 1] > m)) c.bad_index = 1;
    }
    __syncthreads();
    if (c.bad_index) {
        if (tid == 0) {
            res->rounds = -1, res->n_bad_first = 0, res->n_erase = 0, res->pad = 0;
            for (int k = 0; k < 2; ++k) res->lm_iterations[k] = 0, res->lm_rejected[k] = 0;
        }
        return;
    }

    // the job's slices of the workspace
    const Layout L = make_layout(A.batch, A.total_poses, A.total_points, A.total_edges, A.max_local);
    const size_t n_max = L.n;
    double* const S = A.ws + L.sys_d + (size_t)jb * (n_max * n_max + kSysVecs * n_max);
    double* const v_r = S + n_max * n_max;
    double* const v_d = v_r + n_max;
    double* const v_s = v_d + n_max;
    double* const v_y = v_s + n_max;
    double* const v_x = v_y + n_max;
    int* const ibase = reinterpret_cast<int*>(A.ws + L.sys_d + (size_t)A.batch * (n_max * n_max + kSysVecs * n_max));
    int* const ie = ibase + L.edge_i + eo;
    const size_t TE = L.TE;
    auto EI = [ie, TE](int f, int e) -> int& { return ie[(size_t)f * TE + e]; };
    // the strides are the call's totals, the job's offsets are in the base pointers
    ba::View V;
    V.wp = A.ws + L.pose_d + po, V.wl = A.ws + L.point_d + lo, V.we = A.ws + L.edge_d + eo;
    V.ip = ibase + L.pose_i + po, V.il = ibase + L.point_i + lo, V.list = ie + (size_t)IE_LIST * TE;
    V.TP = A.total_poses, V.TM = A.total_points, V.TE = A.total_edges;
    V.edge_pose = epose, V.edge_point = epoint;
    V.cam = A.cam + 5 * po, V.obs = A.obs + 3 * eo, V.inv_sigma2 = A.inv_sigma2 + eo;
    auto level0 = [&EI](int e) { return !EI(IE_LEVEL, e); };  // initializeOptimization(0)'s edges

    // ---------------------------------------------------------------- estimates and structure
    for (int p = tid; p < P; p += T) {  // Converter::toSE3Quat
        double q[4], t[3];
        orbgpu::se3::pose_from_T12(A.Tcw + 12 * (po + p), q, t);
        for (int k = 0; k < 4; ++k) V.PD(P_EST + k, p) = q[k];
        for (int r = 0; r < 3; ++r) V.PD(P_EST + 4 + r, p) = t[r];
        V.PI(IP_COUNT, p) = 0;
    }
    for (int m = tid; m < M; m += T) {
        for (int k = 0; k < 3; ++k) V.LD(L_EST + k, m) = (double)A.Xw[3 * (lo + m) + k];
        V.LI(IL_FIRST, m) = 0, V.LI(IL_END, m) = 0;
    }
    __syncthreads();
    for (int i = tid; i < E; i += T) {  // a point's run of edges
        const int m = epoint[i];
        if (i == 0 || epoint[i - 1] != m) V.LI(IL_FIRST, m) = i;
        if (i == E - 1 || epoint[i + 1] != m) V.LI(IL_END, m) = i + 1;
        EI(IE_LEVEL, i) = 0;
        V.ED(E_CHI, i) = 0.0;
    }
    for (int p = tid; p < P; p += T) {  // the pose-major edge list: count, scan, fill (ascending edges)
        int n = 0;
        for (int i = 0; i < E; ++i) n += epose[i] == p;
        V.PI(IP_COUNT, p) = n;
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int p = 0; p < P; ++p) V.PI(IP_START, p) = s, s += V.PI(IP_COUNT, p);
    }
    __syncthreads();
    for (int p = tid; p < P; p += T) {
        int k = V.PI(IP_START, p);
        for (int i = 0; i < E; ++i)
            if (epose[i] == p) EI(IE_LIST, k++) = i;
    }
    __syncthreads();

    // computeActiveErrors at the trial, or at the estimates with linearizeOplus and the per-edge
    // terms of buildSystem (`build`); returns the robust chi2 over the active edges
    auto evaluate = [&](bool build, bool robust) {
        double acc = 0.0;
        for (int i = tid; i < E; i += T) {
            if (EI(IE_LEVEL, i)) continue;
            double chi2;
            acc += build ? ba::edge_build(V, i, P_EST, L_EST, robust, A.hc, chi2)
                         : ba::edge_chi(V, i, P_TRIAL, L_TRIAL, robust, A.hc, chi2);
            V.ED(E_CHI, i) = chi2;
        }
        return job_total(acc, s_val, s_row, c);
    };

    // the diagonal blocks and right-hand sides of buildSystem: one lane per entry
    auto build_blocks = [&] {
        bool diagonal;
        for (int wi = tid; wi < P * 27; wi += T) {
            const int p = wi / 27, v = wi % 27;
            if (V.PI(IP_FREE, p)) V.PD(P_H + v, p) = ba::pose_entry(V, p, v, level0, diagonal);
        }
        for (int wi = tid; wi < M * 9; wi += T) {
            const int m = wi / 9, v = wi % 9;
            if (V.LI(IL_ACTIVE, m)) V.LD(L_H + v, m) = ba::point_entry(V, m, v, level0, diagonal);
        }
        __syncthreads();
    };

    // BlockSolver::solve at lambda: x of the free poses in v_x, of the active points in L_X; leaves
    // c.solved (0: a pivot of the reduced system was not positive)
    auto solve = [&](double lambda) {
        const int nf = c.nf;
        const int n = 6 * nf;
        for (int m = tid; m < M; m += T)  // Dinv = (Hll + lambda I)^-1, Dinv b_l
            if (V.LI(IL_ACTIVE, m)) ba::point_inverse(V, m, lambda);
        __syncthreads();
        for (int i = tid; i < E; i += T)  // B Dinv of every edge that has a B
            if (!EI(IE_LEVEL, i) && V.PI(IP_FREE, epose[i])) ba::edge_bd(V, i);
        __syncthreads();
        // S = Hpp + lambda I - sum (B Dinv) B^T, upper block triangle.  Half a row of S -- columns
        // s0..s0+2 of every block (a, b >= a) in row r of pose a -- has one owner, which walks the edges
        // of pose a ascending and, inside, the run of the edge's point, and updates its entries in
        // memory: every entry's subtractions keep that order, and the walk is made once per half row
        // (measured: one lane per (a, b, r), each walking the edges of a again, cost 15 ms of a 20 ms
        // iteration at 20 free poses and 12,000 edges)
        for (int wi = tid; wi < nf * 12; wi += T) {
            const int ia = wi / 12, r = (wi % 12) >> 1, s0 = 3 * (wi & 1);
            const int pa = V.PI(IP_HLIST, ia);
            double* const row = S + (size_t)(6 * ia + r) * n;
            for (int ib = ia; ib < nf; ++ib)
                for (int s = s0; s < s0 + 3; ++s) {
                    double h = 0.0;
                    if (ib == ia && s >= r) {
                        h = V.PD(P_H + lm::upper_index<6>(r, s), pa);
                        if (s == r) h = h + lambda;
                    }
                    row[6 * ib + s] = h;
                }
            const int start = V.PI(IP_START, pa), count = V.PI(IP_COUNT, pa);
            for (int k = 0; k < count; ++k) {
                const int e = EI(IE_LIST, start + k);
                if (EI(IE_LEVEL, e)) continue;
                const int m = epoint[e];
                const double d0 = V.ED(E_BD + 3 * r, e), d1 = V.ED(E_BD + 3 * r + 1, e), d2 = V.ED(E_BD + 3 * r + 2, e);
                const int end = V.LI(IL_END, m);
                for (int e2 = V.LI(IL_FIRST, m); e2 < end; ++e2) {
                    const int p2 = epose[e2];
                    if (EI(IE_LEVEL, e2) || !V.PI(IP_FREE, p2)) continue;
                    const int ib = V.PI(IP_HIDX, p2);
                    if (ib < ia) continue;
                    for (int s = s0; s < s0 + 3; ++s)
                        row[6 * ib + s] -= (d0 * V.ED(E_B + 3 * s, e2) + d1 * V.ED(E_B + 3 * s + 1, e2)) + d2 * V.ED(E_B + 3 * s + 2, e2);
                }
            }
        }
        for (int wi = tid; wi < n; wi += T) v_s[wi] = ba::b_schur_entry(V, wi / 6, wi % 6, level0);
        __syncthreads();
        // Cholesky, column by column: A in the upper triangle of S, L below it, its diagonal in v_d
        int ok = 1;
        for (int j = 0; j < n; ++j) {
            for (int i = j + tid; i < n; i += T) {
                double r = S[(size_t)j * n + i];
                for (int k = 0; k < j; ++k) r -= S[(size_t)i * n + k] * S[(size_t)j * n + k];
                v_r[i] = r;
            }
            __syncthreads();
            const double pivot = v_r[j];
            if (!(pivot > 0)) {
                ok = 0;
                break;  // every lane read the same word
            }
            const double d = __dsqrt_rn(pivot);
            for (int i = j + 1 + tid; i < n; i += T) S[(size_t)i * n + j] = v_r[i] / d;
            if (tid == 0) v_d[j] = d;
            __syncthreads();
        }
        if (ok) {
            for (int i = 0; i < n; ++i) {  // L y = b_schur, column oriented: the order of the row sums
                const double yi = v_s[i] / v_d[i];
                if (tid == 0) v_y[i] = yi;
                for (int k = i + 1 + tid; k < n; k += T) v_s[k] -= S[(size_t)k * n + i] * yi;
                __syncthreads();
            }
            if (tid == 0) {  // L^T x = y, rows from the last, each sum ascending
                for (int i = n - 1; i >= 0; --i) {
                    double s = v_y[i];
                    for (int k = i + 1; k < n; ++k) s -= S[(size_t)k * n + i] * v_x[k];
                    v_x[i] = s / v_d[i];
                }
            }
        } else {
            for (int i = tid; i < n; i += T) v_x[i] = 0.0;
        }
        if (tid == 0) c.solved = ok;
        __syncthreads();
        for (int m = tid; m < M; m += T)  // x_l = Dinv (b_l - B^T x_p)
            if (V.LI(IL_ACTIVE, m)) ba::point_x(V, m, v_x, ok != 0, level0);
        __syncthreads();
    };

    // trial = oplus(x) on est: exp(x) * estimate for a free pose, estimate + x for an active point
    auto make_trial = [&] {
        const bool ok = c.solved != 0;
        for (int p = tid; p < P; p += T)
            ba::pose_oplus(V, p, ok && V.PI(IP_FREE, p) ? v_x + 6 * V.PI(IP_HIDX, p) : nullptr);
        for (int m = tid; m < M; m += T) ba::point_oplus(V, m, ok && V.LI(IL_ACTIVE, m));
        __syncthreads();
    };

    // computeScale's sum over the free poses, then the active points
    auto scale_sum = [&](double lambda) {
        double acc = 0.0;
        const int n = 6 * c.nf;
        for (int wi = tid; wi < n; wi += T) {
            const double x = v_x[wi];
            acc += x * (lambda * x + V.PD(P_H + 21 + wi % 6, V.PI(IP_HLIST, wi / 6)));
        }
        for (int wi = tid; wi < 3 * M; wi += T) {
            const int m = wi / 3, k = wi % 3;
            if (!V.LI(IL_ACTIVE, m)) continue;
            const double x = V.LD(L_X + k, m);
            acc += x * (lambda * x + V.LD(L_H + 6 + k, m));
        }
        return job_total(acc, s_val, s_row, c);
    };

    int lm_iterations[2] = {0, 0}, lm_rejected[2] = {0, 0}, n_flag[2] = {0, 0};  // lane 0's
    const int rounds = E ? 2 : 0;
    for (int round = 0; round < rounds; ++round) {
        const bool robust = round == 0;  // the kernels are removed after the first classification
        // initializeOptimization(0): what a level-0 edge touches
        for (int m = tid; m < M; m += T) {
            int act = 0;
            const int end = V.LI(IL_END, m);
            for (int e = V.LI(IL_FIRST, m); e < end; ++e) act |= !EI(IE_LEVEL, e);
            V.LI(IL_ACTIVE, m) = act;
        }
        for (int p = tid; p < P; p += T) {
            int act = 0;
            const int start = V.PI(IP_START, p), count = V.PI(IP_COUNT, p);
            for (int k = 0; k < count; ++k) act |= !EI(IE_LEVEL, EI(IE_LIST, start + k));
            V.PI(IP_FREE, p) = act && p < NL && !A.fixed[po + p];
        }
        __syncthreads();
        if (tid == 0) {
            int nf = 0, na = 0;
            for (int p = 0; p < P; ++p) {
                V.PI(IP_HIDX, p) = -1;
                if (V.PI(IP_FREE, p)) V.PI(IP_HIDX, p) = nf, V.PI(IP_HLIST, nf) = p, ++nf;
            }
            for (int m = 0; m < M; ++m) na += V.LI(IL_ACTIVE, m);
            c.nf = nf, c.n_active = na, c.done = 0, c.n_flag = 0;
            lm::run_start(c.run);
        }
        __syncthreads();

        if (c.nf + c.n_active > 0) {  // optimize() returns at once without an active vertex
            const int max_iter = kIterations[round];
            for (int it = 0; it < max_iter; ++it) {
                const double chi = evaluate(true, robust);
                build_blocks();
                if (it == 0) {  // computeLambdaInit: the maximum is exact in any order
                    double mx = 0.0;
                    for (int wi = tid; wi < 6 * c.nf; wi += T) {
                        const int j = wi % 6;
                        const double a = fabs(V.PD(P_H + lm::upper_index<6>(j, j), V.PI(IP_HLIST, wi / 6)));
                        mx = a < mx ? mx : a;
                    }
                    for (int wi = tid; wi < 3 * M; wi += T) {
                        const int m = wi / 3, j = wi % 3;
                        if (!V.LI(IL_ACTIVE, m)) continue;
                        const double a = fabs(V.LD(L_H + (j == 0 ? 0 : (j == 1 ? 3 : 5)), m));
                        mx = a < mx ? mx : a;
                    }
                    s_val[tid] = mx;
                    __syncthreads();
                    if (tid == 0) {
                        double all = 0.0;
                        for (int k = 0; k < T; ++k) all = s_val[k] < all ? all : s_val[k];
                        lm::run_init_lambda(c.run, all);
                    }
                }
                if (tid == 0) lm::run_begin_iteration(c.run, chi);
                __syncthreads();
                for (int trial = 0; trial < lm::kMaxTrials; ++trial) {
                    const double lambda = c.run.lambda;
                    solve(lambda);
                    make_trial();
                    const double tmp_chi = evaluate(false, robust);
                    const double ssum = scale_sum(lambda);
                    if (tid == 0) {
                        c.accepted = lm::run_judge(c.run, c.solved != 0, tmp_chi, ssum) ? 1 : 0;
                        c.more = lm::run_more_trials(c.run) ? 1 : 0;
                    }
                    __syncthreads();
                    if (c.accepted) {
                        for (int wi = tid; wi < 7 * P; wi += T) V.PD(P_EST + wi % 7, wi / 7) = V.PD(P_TRIAL + wi % 7, wi / 7);
                        for (int wi = tid; wi < 3 * M; wi += T) V.LD(L_EST + wi % 3, wi / 3) = V.LD(L_TRIAL + wi % 3, wi / 3);
                    }
                    __syncthreads();
                    if (!c.more) break;
                }
                if (tid == 0) c.done = lm::run_end_iteration(c.run, max_iter) ? 1 : 0;
                __syncthreads();
                if (c.done) break;
            }
        }

        // the test of Optimizer.cpp:773-804 / :818-847: chi2() as the edge holds it, depth at the kept estimates
        int flagged = 0;
        for (int i = tid; i < E; i += T) {
            ba::EdgeAt g;
            ba::edge_error(V, i, P_EST, L_EST, g);
            const bool flag = V.ED(E_CHI, i) > (g.stereo ? 7.815 : 5.991) || !(g.z > 0.0);
            if (round == 0)
                EI(IE_LEVEL, i) = flag ? 1 : 0;
            else
                A.erase[eo + i] = flag ? 1 : 0;
            flagged += flag;
        }
        if (flagged) atomicAdd(&c.n_flag, flagged);  // integers: any order gives the same sum
        __syncthreads();
        if (tid == 0) {
            lm_iterations[round] = c.run.iter;
            lm_rejected[round] = c.run.rejected;
            n_flag[round] = c.n_flag;
        }
        __syncthreads();
    }

    for (int p = tid; p < NL; p += T) {  // Converter::toCvMat(SE3Quat) of every local pose
        const double q[4] = {V.PD(P_EST, p), V.PD(P_EST + 1, p), V.PD(P_EST + 2, p), V.PD(P_EST + 3, p)};
        const double t[3] = {V.PD(P_EST + 4, p), V.PD(P_EST + 5, p), V.PD(P_EST + 6, p)};
        lm::write_T16(q, t, 1.0, A.Tcw_out + 16 * ((size_t)c.oo + p));
    }
    for (int wi = tid; wi < 3 * M; wi += T) A.Xw_out[3 * lo + wi] = (float)V.LD(L_EST + wi % 3, wi / 3);
    if (tid == 0) {
        res->rounds = rounds, res->n_bad_first = n_flag[0], res->n_erase = n_flag[1], res->pad = 0;
        for (int k = 0; k < 2; ++k) res->lm_iterations[k] = lm_iterations[k], res->lm_rejected[k] = lm_rejected[k];
    }
}

int check_args(int batch, int total_poses, int total_local, int total_points, int total_edges, int max_local,
               bool jobs_and_results, bool pose_arrays, bool local_arrays, bool point_arrays, bool edge_arrays) {
    using orbgpu::fail;
    if (batch < 0 || total_poses < 0 || total_local < 0 || total_points < 0 || total_edges < 0 || max_local < 0)
        return fail(ORBGPU_ERR_ARG, "negative batch, total or max_local");
    if (batch > 0 && !jobs_and_results) return fail(ORBGPU_ERR_ARG, "null jobs or results");
    if (batch > 0 && total_poses > 0 && !pose_arrays) return fail(ORBGPU_ERR_ARG, "null pose array");
    if (batch > 0 && total_local > 0 && !local_arrays) return fail(ORBGPU_ERR_ARG, "null local pose output");
    if (batch > 0 && total_points > 0 && !point_arrays) return fail(ORBGPU_ERR_ARG, "null point array");
    if (batch > 0 && total_edges > 0 && !edge_arrays) return fail(ORBGPU_ERR_ARG, "null edge array");
    return ORBGPU_OK;
}

}  // namespace

extern "C" size_t orbgpu_local_ba_workspace_bytes(int batch, int total_poses, int total_points, int total_edges,
                                                  int max_local) {
    if (batch < 0 || total_poses < 0 || total_points < 0 || total_edges < 0 || max_local < 0) return 0;
    return make_layout(batch, total_poses, total_points, total_edges, max_local).bytes;
}

extern "C" int orbgpu_local_ba_batch_device(int batch, const orbgpu_localba_job* d_jobs, int total_poses,
                                            int total_local, int total_points, int total_edges, int max_local,
                                            const float* d_Tcw, const uint8_t* d_fixed, const float* d_cam,
                                            const float* d_Xw, const int* d_edge_pose, const int* d_edge_point,
                                            const float* d_obs, const float* d_inv_sigma2, float* d_Tcw_out,
                                            float* d_Xw_out, uint8_t* d_erase, orbgpu_localba_result* d_results,
                                            void* d_workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_args(batch, total_poses, total_local, total_points, total_edges, max_local,
                            d_jobs && d_results, d_Tcw && d_fixed && d_cam, d_Tcw_out, d_Xw && d_Xw_out,
                            d_edge_pose && d_edge_point && d_obs && d_inv_sigma2 && d_erase))
        return rc;
    if (batch == 0) return ORBGPU_OK;
    if (!d_workspace || ((uintptr_t)d_workspace & 7) ||
        workspace_bytes < orbgpu_local_ba_workspace_bytes(batch, total_poses, total_points, total_edges, max_local))
        return orbgpu::fail(ORBGPU_ERR_ARG, "null, misaligned or too small workspace");
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    Args a;
    a.jobs = d_jobs, a.batch = batch, a.total_poses = total_poses, a.total_local = total_local;
    a.total_points = total_points, a.total_edges = total_edges, a.max_local = max_local;
    a.Tcw = d_Tcw, a.cam = d_cam, a.Xw = d_Xw, a.obs = d_obs, a.inv_sigma2 = d_inv_sigma2, a.fixed = d_fixed;
    a.edge_pose = d_edge_pose, a.edge_point = d_edge_point;
    a.Tcw_out = d_Tcw_out, a.Xw_out = d_Xw_out, a.erase = d_erase, a.results = d_results;
    a.ws = static_cast<double*>(d_workspace);
    a.hc = orbgpu::proj_edge::huber_constants(5.991, 7.815);  // Optimizer.cpp:666-667
    hipLaunchKernelGGL(localba_kernel, dim3(batch), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_local_ba_batch(int batch, const orbgpu_localba_job* jobs, int total_poses, int total_local,
                                     int total_points, int total_edges, int max_local, const float* Tcw,
                                     const uint8_t* fixed, const float* cam, const float* Xw, const int* edge_pose,
                                     const int* edge_point, const float* obs, const float* inv_sigma2,
                                     float* Tcw_out, float* Xw_out, uint8_t* erase, orbgpu_localba_result* results,
                                     void* d_workspace, size_t workspace_bytes) {
    using namespace orbgpu;
    int rc = check_args(batch, total_poses, total_local, total_points, total_edges, max_local, jobs && results,
                        Tcw && fixed && cam, Tcw_out, Xw && Xw_out,
                        edge_pose && edge_point && obs && inv_sigma2 && erase);
    if (rc) return rc;
    for (int b = 0; b < batch; ++b) {
        const orbgpu_localba_job& j = jobs[b];
        if (!job_ranges_ok(j, total_poses, total_local, total_points, total_edges, max_local))
            return fail(ORBGPU_ERR_ARG, "job " + std::to_string(b) + " is out of the array bounds");
        for (int i = 0; i < j.n_edges; ++i) {
            const int p = edge_pose[j.edge_offset + i], m = edge_point[j.edge_offset + i];
            if (p < 0 || p >= j.n_poses || m < 0 || m >= j.n_points)
                return fail(ORBGPU_ERR_ARG, "job " + std::to_string(b) + ": an edge index is out of range");
            if (i > 0 && edge_point[j.edge_offset + i - 1] > m)
                return fail(ORBGPU_ERR_ARG, "job " + std::to_string(b) + ": point indices decrease");
        }
    }
    if (batch == 0) return ORBGPU_OK;
    const size_t need = orbgpu_local_ba_workspace_bytes(batch, total_poses, total_points, total_edges, max_local);
    if (d_workspace && (((uintptr_t)d_workspace & 7) || workspace_bytes < need))
        return fail(ORBGPU_ERR_ARG, "misaligned or too small workspace");
    if ((rc = check_device())) return rc;
    DevBuf<uint8_t> own;
    if (!d_workspace) {
        if ((rc = dalloc(own, need))) return rc;
        d_workspace = own.get();
        workspace_bytes = need;
    }
    const size_t tp = (size_t)total_poses, tl = (size_t)total_local, tm = (size_t)total_points, te = (size_t)total_edges;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    HostCall call(*ctx);
    const orbgpu_localba_job* dj;
    const float *dT, *dcam, *dX, *dobs, *dw;
    const uint8_t* dfix;
    const int *dep, *del;
    float *dTo, *dXo;
    uint8_t* der;
    orbgpu_localba_result* dr;
    rc = call.run([&](HostCall& A) {
        dj = A.in(jobs, (size_t)batch);
        dT = A.in(Tcw, 12 * tp);
        dfix = A.in(fixed, tp);
        dcam = A.in(cam, 5 * tp);
        dX = A.in(Xw, 3 * tm);
        dep = A.in(edge_pose, te);
        del = A.in(edge_point, te);
        dobs = A.in(obs, 3 * te);
        dw = A.in(inv_sigma2, te);
        // outputs outside every job's ranges keep the caller's values
        dTo = A.inout(Tcw_out, 16 * tl);
        dXo = A.inout(Xw_out, 3 * tm);
        der = A.inout(erase, te);
        dr = A.out<orbgpu_localba_result>((size_t)batch);
    });
    if (rc) return rc;
    rc = orbgpu_local_ba_batch_device(batch, dj, total_poses, total_local, total_points, total_edges, max_local, dT,
                                      dfix, dcam, dX, dep, del, dobs, dw, dTo, dXo, der, dr, d_workspace,
                                      workspace_bytes, ctx->stream);
    if (rc) return rc;
    call.fetch(dr, results, sizeof(*dr) * batch);
    call.fetch(dTo, Tcw_out, sizeof(float) * 16 * tl);
    call.fetch(dXo, Xw_out, sizeof(float) * 3 * tm);
    call.fetch(der, erase, te);
    rc = call.finish();  // synchronises: the workspace is free again
    return rc;
}
