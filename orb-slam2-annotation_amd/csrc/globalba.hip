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
// kernels keep their own bodies over this file's Args: the per-item arithmetic
// is ba_schur_device.h's text, and moving the kernels onto its view measured
// 0.5-0.9 % slower in ba_schur for a reason that was not found.
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
#include "ba_schur_device.h"
#include "chol_blocked.h"
#include "host_common.h"
#include "host_ctx.h"
#include "wholechip_lm.h"

namespace {

namespace lm = orbgpu::lm;
namespace wc = orbgpu::wholechip;
using namespace orbgpu::ba;  // the field offsets
using lm::upper_jk;
using orbgpu::se3::quat_to_R;
using orbgpu::se3::se3_exp_times;
using wc::block_total;
using wc::blocks_for;
using wc::global_tid;
using wc::HostRec;
using wc::kCtlBytes;

constexpr int kThreads = 256;
constexpr int kEdgeD = 67, kPointI = 2;  // doubles per edge, ints per point: ba_schur_device.h's fields alone

// the optimisation's state on the device (wholechip::CtlBase's members and computeLambdaInit's maximum);
// zeroed by the call, then written by one lane of one kernel at a time
struct Ctl {
    lm::Run run;
    unsigned long long max_bits;  // computeLambdaInit's maximum, as bits
    double first_chi;
    int bad, fail, nf, n_active;
};
static_assert(sizeof(Ctl) <= kCtlBytes, "Ctl outgrew its slot");

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

// what every kernel gets
struct Args {
    int P, M, E, robust;
    const float *Tcw, *cam, *Xw, *obs, *inv_sigma2;
    const uint8_t* fixed;
    const int *edge_pose, *edge_point;
    float *Tcw_out, *Xw_out;
    Ctl* ctl;
    HostRec* rec;
    double *wp, *wl, *we, *S, *x, *chi_part, *scale_part;
    int *ip, *il, *ie;
    int n_chi, n_scale;
    double delta_mono, delta_stereo, dsqr_mono, dsqr_stereo;
};

#define PD(f, p) A.wp[(size_t)(f) * A.P + (p)]
#define LD(f, m) A.wl[(size_t)(f) * A.M + (m)]
#define ED(f, e) A.we[(size_t)(f) * A.E + (e)]
#define PI(f, p) A.ip[(size_t)(f) * A.P + (p)]
#define LI(f, m) A.il[(size_t)(f) * A.M + (m)]

// ------------------------------------------------------------------ once per call: check and structure

// an edge index out of range or edge_point decreasing: nothing else may index with these arrays
__global__ __launch_bounds__(kThreads) void ba_check(Args A) {
    const size_t i = global_tid();
    if (i >= (size_t)A.E) return;
    const int p = A.edge_pose[i], m = A.edge_point[i];
    if (p < 0 || p >= A.P || m < 0 || m >= A.M || (i > 0 && A.edge_point[i - 1] > m)) A.ctl->bad = 1;
}

// Converter::toSE3Quat of every pose, every point widened; the counters cleared
__global__ __launch_bounds__(kThreads) void ba_init(Args A) {
    const size_t i = global_tid();
    if (i < (size_t)A.P) {
        const int p = (int)i;
        double q[4], t[3];
        orbgpu::se3::pose_from_T12(A.Tcw + 12 * i, q, t);
        for (int k = 0; k < 4; ++k) PD(P_EST + k, p) = q[k];
        for (int r = 0; r < 3; ++r) PD(P_EST + 4 + r, p) = t[r];
        PI(IP_COUNT, p) = 0;
    }
    if (i < (size_t)A.M) {
        const int m = (int)i;
        for (int k = 0; k < 3; ++k) LD(L_EST + k, m) = (double)A.Xw[3 * i + k];
        LI(IL_FIRST, m) = 0, LI(IL_END, m) = 0;
    }
}

// a point's run of edges, the number of edges of every pose and of points with an edge (integer atomics)
__global__ __launch_bounds__(kThreads) void ba_runs(Args A) {
    if (A.ctl->bad) return;
    const size_t gi = global_tid();
    if (gi >= (size_t)A.E) return;
    const int i = (int)gi, m = A.edge_point[i];
    if (i == 0 || A.edge_point[i - 1] != m) LI(IL_FIRST, m) = i;
    if (i == A.E - 1 || A.edge_point[i + 1] != m) {
        LI(IL_END, m) = i + 1;
        atomicAdd(&A.ctl->n_active, 1);
    }
    atomicAdd(&PI(IP_COUNT, A.edge_pose[i]), 1);
}

// where each pose's edge list starts, which poses are free, their order in the reduced system; one lane
__global__ void ba_scan(Args A) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    HostRec* rec = A.rec;
    rec->bad = A.ctl->bad;
    if (A.ctl->bad) {
        rec->nf = 0, rec->n_active = 0;
        __threadfence_system();
        return;
    }
    int s = 0, nf = 0;
    for (int p = 0; p < A.P; ++p) {
        const int count = PI(IP_COUNT, p);
        PI(IP_START, p) = s;
        s += count;
        const int is_free = count > 0 && !A.fixed[p];
        PI(IP_FREE, p) = is_free;
        PI(IP_HIDX, p) = -1;
        if (is_free) PI(IP_HIDX, p) = nf, PI(IP_HLIST, nf) = p, ++nf;
    }
    A.ctl->nf = nf;
    rec->nf = nf, rec->n_active = A.ctl->n_active;
    __threadfence_system();
}

// the pose-major edge list, ascending: one wave per pose scans the edges 64 at a time
__global__ __launch_bounds__(kThreads) void ba_lists(Args A) {
    if (A.ctl->bad) return;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (p >= A.P) return;  // a whole wave
    int before = PI(IP_START, p);
    for (int i0 = 0; i0 < A.E; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < A.E && A.edge_pose[i] == p;
        const unsigned long long mask = __ballot(mine);
        if (mine) A.ie[before + (int)__popcll(mask & ((1ull << lane) - 1))] = i;
        before += (int)__popcll(mask);
    }
}

// ------------------------------------------------------------------ per iteration and per trial: the edges

// computeError of edge i at the estimates in field est_p / est_l: chi2, camera-frame point
__device__ inline double edge_error(const Args& A, int i, int est_p, int est_l, double& x, double& y, double& z,
                                    double (&e)[3], double (&q)[4], double& w, bool& stereo, const float*& cam) {
    const int p = A.edge_pose[i], m = A.edge_point[i];
    double t[3];
    for (int k = 0; k < 4; ++k) q[k] = PD(est_p + k, p);
    for (int k = 0; k < 3; ++k) t[k] = PD(est_p + 4 + k, p);
    double r0, r1, r2;
    lm::quat_rotate(q, LD(est_l, m), LD(est_l + 1, m), LD(est_l + 2, m), r0, r1, r2);
    x = r0 + t[0], y = r1 + t[1], z = r2 + t[2];
    cam = A.cam + 5 * (size_t)p;
    const double fx = (double)cam[0], fy = (double)cam[1], cx = (double)cam[2], cy = (double)cam[3];
    const float* ob = A.obs + 3 * (size_t)i;
    w = (double)A.inv_sigma2[i];
    stereo = ob[2] >= 0.0f;
    if (stereo) {
        const double bf = (double)cam[4];
        const double invzf = (double)(float)(1.0 / z);  // const float invz = 1.0f / trans_xyz[2]
        const double us = (x * invzf) * fx + cx;
        const double vs = (y * invzf) * fy + cy;
        const double rs = us - bf * invzf;
        e[0] = (double)ob[0] - us;
        e[1] = (double)ob[1] - vs;
        e[2] = (double)ob[2] - rs;
        return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
    }
    e[0] = (double)ob[0] - ((x / z) * fx + cx);
    e[1] = (double)ob[1] - ((y / z) * fy + cy);
    e[2] = 0.0;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// computeActiveErrors (+ linearizeOplus and the per-edge terms of buildSystem when kBuild) at the
// estimates (kBuild) or the trial; the workgroup's robust chi2 goes to chi_part[blockIdx.x]
template <bool kBuild>
__global__ __launch_bounds__(kThreads) void ba_edges(Args A) {
    __shared__ double s_val[kThreads];
    __shared__ double s_row[16];
    if (!kBuild && A.ctl->fail) return;
    const size_t gi = global_tid();
    double rho0 = 0.0;
    if (gi < (size_t)A.E) {
        const int i = (int)gi;
        double x, y, z, e[3], q[4], w;
        bool stereo;
        const float* cam;
        const double chi2 = edge_error(A, i, kBuild ? P_EST : P_TRIAL, kBuild ? L_EST : L_TRIAL, x, y, z, e, q, w, stereo,
                                       cam);
        double rho1 = 1.0;
        rho0 = chi2;
        if (A.robust)
            lm::huber(chi2, stereo ? A.delta_stereo : A.delta_mono, stereo ? A.dsqr_stereo : A.dsqr_mono, rho0, rho1);
        if (kBuild) {
            const double fx = (double)cam[0], fy = (double)cam[1], bf = (double)cam[4];
            double R[3][3], Jl[3][3], Jp[3][6];
            quat_to_R(q, R);
            const double z_2 = z * z;
            if (stereo) {
                for (int col = 0; col < 3; ++col) {
                    Jl[0][col] = ((-fx) * R[0][col]) / z + ((fx * x) * R[2][col]) / z_2;
                    Jl[1][col] = ((-fy) * R[1][col]) / z + ((fy * y) * R[2][col]) / z_2;
                    Jl[2][col] = Jl[0][col] - (bf * R[2][col]) / z_2;
                }
            } else {  // -1./z * tmp * R
                const double s = -1.0 / z;
                const double t00 = s * fx, t01 = s * 0.0, t02 = s * (((-x) / z) * fx);
                const double t10 = s * 0.0, t11 = s * fy, t12 = s * (((-y) / z) * fy);
                for (int col = 0; col < 3; ++col) {
                    Jl[0][col] = (t00 * R[0][col] + t01 * R[1][col]) + t02 * R[2][col];
                    Jl[1][col] = (t10 * R[0][col] + t11 * R[1][col]) + t12 * R[2][col];
                    Jl[2][col] = 0.0;
                }
            }
            Jp[0][0] = ((x * y) / z_2) * fx;
            Jp[0][1] = (-(1.0 + (x * x) / z_2)) * fx;
            Jp[0][2] = (y / z) * fx;
            Jp[0][3] = (-1.0 / z) * fx;
            Jp[0][4] = 0.0;
            Jp[0][5] = (x / z_2) * fx;
            Jp[1][0] = (1.0 + (y * y) / z_2) * fy;
            Jp[1][1] = (((-x) * y) / z_2) * fy;
            Jp[1][2] = ((-x) / z) * fy;
            Jp[1][3] = 0.0;
            Jp[1][4] = (-1.0 / z) * fy;
            Jp[1][5] = (y / z_2) * fy;
            if (stereo) {
                Jp[2][0] = Jp[0][0] - (bf * y) / z_2;
                Jp[2][1] = Jp[0][1] + (bf * x) / z_2;
                Jp[2][2] = Jp[0][2];
                Jp[2][3] = Jp[0][3];
                Jp[2][4] = 0.0;
                Jp[2][5] = Jp[0][5] - bf / z_2;
            } else {
                for (int k = 0; k < 6; ++k) Jp[2][k] = 0.0;
            }
            const double Wt = rho1 * w;
            ED(E_W, i) = Wt;
            for (int r = 0; r < 3; ++r) {
                ED(E_OMR + r, i) = rho1 * (-(w * e[r]));
                for (int k = 0; k < 6; ++k) ED(E_JP + 6 * r + k, i) = Jp[r][k];
                for (int k = 0; k < 3; ++k) ED(E_JL + 3 * r + k, i) = Jl[r][k];
            }
            for (int a = 0; a < 6; ++a)
                for (int col = 0; col < 3; ++col)
                    ED(E_B + 3 * a + col, i) = ((Wt * Jp[0][a]) * Jl[0][col] + (Wt * Jp[1][a]) * Jl[1][col]) +
                                               (Wt * Jp[2][a]) * Jl[2][col];
        }
    }
    const double total = block_total(rho0, s_val, s_row);
    if (threadIdx.x == 0) A.chi_part[blockIdx.x] = total;
}

__device__ inline void note_diagonal(const Args& A, double h) {
    atomicMax(&A.ctl->max_bits, (unsigned long long)__double_as_longlong(fabs(h)));
}

// the diagonal blocks and right-hand sides of buildSystem: one lane per entry, 27 per pose, then 9
// per point; in the first iteration the diagonal entries enter computeLambdaInit's maximum
__global__ __launch_bounds__(kThreads) void ba_vertex_sums(Args A, int first) {
    const size_t gi = global_tid();
    const size_t n_pose = (size_t)A.P * 27;
    if (gi < n_pose) {
        const int p = (int)(gi / 27), v = (int)(gi % 27);
        if (!PI(IP_FREE, p)) return;
        const int start = PI(IP_START, p), count = PI(IP_COUNT, p);
        double acc = 0.0;
        if (v < 21) {
            int j, k;
            upper_jk<6>(v, j, k);
            for (int s = 0; s < count; ++s) {
                const int e = A.ie[start + s];
                const double Wt = ED(E_W, e);
                acc += ((Wt * ED(E_JP + j, e)) * ED(E_JP + k, e) + (Wt * ED(E_JP + 6 + j, e)) * ED(E_JP + 6 + k, e)) +
                       (Wt * ED(E_JP + 12 + j, e)) * ED(E_JP + 12 + k, e);
            }
            if (first && j == k) note_diagonal(A, acc);
        } else {
            const int j = v - 21;
            for (int s = 0; s < count; ++s) {
                const int e = A.ie[start + s];
                acc += (ED(E_JP + j, e) * ED(E_OMR, e) + ED(E_JP + 6 + j, e) * ED(E_OMR + 1, e)) +
                       ED(E_JP + 12 + j, e) * ED(E_OMR + 2, e);
            }
        }
        PD(P_H + v, p) = acc;
        return;
    }
    const size_t li = gi - n_pose;
    if (li >= (size_t)A.M * 9) return;
    const int m = (int)(li / 9), v = (int)(li % 9);
    const int begin = LI(IL_FIRST, m), end = LI(IL_END, m);
    if (end <= begin) return;
    double acc = 0.0;
    if (v < 6) {
        int j, k;
        upper_jk<3>(v, j, k);
        for (int e = begin; e < end; ++e) {
            const double Wt = ED(E_W, e);
            acc += ((Wt * ED(E_JL + j, e)) * ED(E_JL + k, e) + (Wt * ED(E_JL + 3 + j, e)) * ED(E_JL + 3 + k, e)) +
                   (Wt * ED(E_JL + 6 + j, e)) * ED(E_JL + 6 + k, e);
        }
        if (first && j == k) note_diagonal(A, acc);
    } else {
        const int j = v - 6;
        for (int e = begin; e < end; ++e)
            acc += (ED(E_JL + j, e) * ED(E_OMR, e) + ED(E_JL + 3 + j, e) * ED(E_OMR + 1, e)) +
                   ED(E_JL + 6 + j, e) * ED(E_OMR + 2, e);
    }
    LD(L_H + v, m) = acc;
}

// the iteration begins: the robust chi2 at the kept estimates, computeLambdaInit in the first
__global__ void ba_begin(Args A, int first) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Ctl& c = *A.ctl;
    wc::begin_iteration(c, A.chi_part, A.n_chi, first, [&c](lm::Run& run) {
        lm::run_init_lambda(run, __longlong_as_double((long long)c.max_bits));
    });
}

// Dinv = (Hll + lambda I)^-1 from cofactors and Dinv b_l, one lane per point
__global__ __launch_bounds__(kThreads) void ba_point_inverse(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.M) return;
    const int m = (int)gi;
    if (LI(IL_END, m) <= LI(IL_FIRST, m)) return;
    const double lambda = A.ctl->run.lambda;
    const double a = LD(L_H, m) + lambda, b = LD(L_H + 1, m), cc = LD(L_H + 2, m);
    const double d = LD(L_H + 3, m) + lambda, e = LD(L_H + 4, m), f = LD(L_H + 5, m) + lambda;
    const double c00 = d * f - e * e, c01 = cc * e - b * f, c02 = b * e - cc * d;
    const double c11 = a * f - cc * cc, c12 = b * cc - a * e, c22 = a * d - b * b;
    const double inv = 1.0 / ((a * c00 + b * c01) + cc * c02);
    const double D[3][3] = {{c00 * inv, c01 * inv, c02 * inv}, {c01 * inv, c11 * inv, c12 * inv}, {c02 * inv, c12 * inv, c22 * inv}};
    LD(L_DINV, m) = D[0][0], LD(L_DINV + 1, m) = D[0][1], LD(L_DINV + 2, m) = D[0][2];
    LD(L_DINV + 3, m) = D[1][1], LD(L_DINV + 4, m) = D[1][2], LD(L_DINV + 5, m) = D[2][2];
    const double b0 = LD(L_H + 6, m), b1 = LD(L_H + 7, m), b2 = LD(L_H + 8, m);
    for (int k = 0; k < 3; ++k) LD(L_V + k, m) = (D[k][0] * b0 + D[k][1] * b1) + D[k][2] * b2;
}

// Dinv (row-major, symmetric) of point m from its six stored entries
__device__ inline void load_dinv(const Args& A, int m, double (&D)[3][3]) {
    D[0][0] = LD(L_DINV, m), D[0][1] = LD(L_DINV + 1, m), D[0][2] = LD(L_DINV + 2, m);
    D[1][1] = LD(L_DINV + 3, m), D[1][2] = LD(L_DINV + 4, m), D[2][2] = LD(L_DINV + 5, m);
    D[1][0] = D[0][1], D[2][0] = D[0][2], D[2][1] = D[1][2];
}

// B Dinv of every edge that has a B (its pose is free), one lane per edge
__global__ __launch_bounds__(kThreads) void ba_edge_bd(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.E) return;
    const int i = (int)gi;
    if (!PI(IP_FREE, A.edge_pose[i])) return;
    double D[3][3];
    load_dinv(A, A.edge_point[i], D);
    for (int a = 0; a < 6; ++a) {
        const double b0 = ED(E_B + 3 * a, i), b1 = ED(E_B + 3 * a + 1, i), b2 = ED(E_B + 3 * a + 2, i);
        for (int k = 0; k < 3; ++k) ED(E_BD + 3 * a + k, i) = (b0 * D[0][k] + b1 * D[1][k]) + b2 * D[2][k];
    }
}

// S = Hpp + lambda I - sum (B Dinv) B^T and b_schur = b_p - sum B (Dinv b_l).  The matrix is kept as
// its lower triangle, rows of n = 6 nf doubles, b_schur being row n: entry (r, s) of block (a, b >= a)
// lives at row 6 b + s, column 6 a + r.  36 lanes per block; then one lane per entry of b_schur.
__global__ __launch_bounds__(kThreads) void ba_schur(Args A) {
    const int nf = A.ctl->nf;
    const size_t n = 6 * (size_t)nf;
    const size_t gi = global_tid();
    const size_t n_block_lanes = (size_t)nf * nf * 36;
    const int* epoint = A.edge_point;
    if (gi < n_block_lanes) {
        const size_t blk = gi / 36;
        const int l = (int)(gi % 36), r = l / 6, s = l % 6;
        const int ia = (int)(blk / nf), ib = (int)(blk % nf);
        if (ib < ia || (ib == ia && s < r)) return;
        const int pa = PI(IP_HLIST, ia), pb = PI(IP_HLIST, ib);
        double h = 0.0;
        if (ib == ia) {
            h = PD(P_H + lm::upper_index<6>(r, s), pa);
            if (s == r) h = h + A.ctl->run.lambda;
        }
        const int sa = PI(IP_START, pa), ca = PI(IP_COUNT, pa), sb = PI(IP_START, pb), cb = PI(IP_COUNT, pb);
        int jb = 0;
        for (int ka = 0; ka < ca; ++ka) {  // the two lists ascend in the edge index, so in the point index
            const int e = A.ie[sa + ka], m = epoint[e];
            while (jb < cb && epoint[A.ie[sb + jb]] < m) ++jb;
            if (jb >= cb) break;
            if (epoint[A.ie[sb + jb]] != m) continue;
            const double d0 = ED(E_BD + 3 * r, e), d1 = ED(E_BD + 3 * r + 1, e), d2 = ED(E_BD + 3 * r + 2, e);
            for (int j2 = jb; j2 < cb; ++j2) {
                const int e2 = A.ie[sb + j2];
                if (epoint[e2] != m) break;
                h -= (d0 * ED(E_B + 3 * s, e2) + d1 * ED(E_B + 3 * s + 1, e2)) + d2 * ED(E_B + 3 * s + 2, e2);
            }
        }
        A.S[((size_t)6 * ib + s) * n + (size_t)6 * ia + r] = h;
        return;
    }
    const size_t wi = gi - n_block_lanes;
    if (wi >= n) return;
    const int ia = (int)(wi / 6), j = (int)(wi % 6);
    const int pa = PI(IP_HLIST, ia);
    const int start = PI(IP_START, pa), count = PI(IP_COUNT, pa);
    double coef = 0.0;
    for (int k = 0; k < count; ++k) {
        const int e = A.ie[start + k], m = epoint[e];
        coef += (ED(E_B + 3 * j, e) * LD(L_V, m) + ED(E_B + 3 * j + 1, e) * LD(L_V + 1, m)) +
                ED(E_B + 3 * j + 2, e) * LD(L_V + 2, m);
    }
    A.S[n * n + wi] = PD(P_H + 21 + j, pa) - coef;
}

// ------------------------------------------------------------------ the blocked Cholesky: chol_blocked.h

// what its kernels read of the workspace
struct SystemView {
    double *S, *x;
    int* fail;
    const int* nf;
    __device__ size_t n() const { return 6 * (size_t)*nf; }
};

// ------------------------------------------------------------------ the step, the trial, the judge

// x_l = Dinv (b_l - B^T x_p), one lane per point; zero after a failed solve
__global__ __launch_bounds__(kThreads) void ba_point_x(Args A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.M) return;
    const int m = (int)gi;
    const int begin = LI(IL_FIRST, m), end = LI(IL_END, m);
    if (end <= begin) return;
    if (A.ctl->fail) {
        for (int k = 0; k < 3; ++k) LD(L_X + k, m) = 0.0;
        return;
    }
    double t[3] = {LD(L_H + 6, m), LD(L_H + 7, m), LD(L_H + 8, m)};
    for (int e = begin; e < end; ++e) {
        const int p = A.edge_pose[e];
        if (!PI(IP_FREE, p)) continue;
        const double* xp = A.x + 6 * (size_t)PI(IP_HIDX, p);
        for (int k = 0; k < 3; ++k) {
            double dot = ED(E_B + k, e) * xp[0];
            for (int a = 1; a < 6; ++a) dot = dot + ED(E_B + 3 * a + k, e) * xp[a];
            t[k] -= dot;
        }
    }
    double D[3][3];
    load_dinv(A, m, D);
    for (int k = 0; k < 3; ++k) LD(L_X + k, m) = (D[k][0] * t[0] + D[k][1] * t[1]) + D[k][2] * t[2];
}

// trial = oplus(x) on the estimates, one lane per vertex (the poses, then the points), and the
// vertex's terms of computeScale's sum; the workgroup's sum goes to scale_part[blockIdx.x]
__global__ __launch_bounds__(kThreads) void ba_trial(Args A) {
    __shared__ double s_val[kThreads];
    __shared__ double s_row[16];
    const size_t gi = global_tid();
    const bool ok = !A.ctl->fail;
    const double lambda = A.ctl->run.lambda;
    double acc = 0.0;
    if (gi < (size_t)A.P) {
        const int p = (int)gi;
        double q[4], t[3];
        for (int k = 0; k < 4; ++k) q[k] = PD(P_EST + k, p);
        for (int k = 0; k < 3; ++k) t[k] = PD(P_EST + 4 + k, p);
        if (ok && PI(IP_FREE, p)) {
            const double* xp = A.x + 6 * (size_t)PI(IP_HIDX, p);
            const double x[6] = {xp[0], xp[1], xp[2], xp[3], xp[4], xp[5]};
            double oq[4], ot[3];
            se3_exp_times(q, t, x, oq, ot);
            for (int k = 0; k < 4; ++k) q[k] = oq[k];
            for (int k = 0; k < 3; ++k) t[k] = ot[k];
            for (int k = 0; k < 6; ++k) acc += x[k] * (lambda * x[k] + PD(P_H + 21 + k, p));
        }
        for (int k = 0; k < 4; ++k) PD(P_TRIAL + k, p) = q[k];
        for (int k = 0; k < 3; ++k) PD(P_TRIAL + 4 + k, p) = t[k];
    } else if (gi < (size_t)A.P + A.M) {
        const int m = (int)(gi - A.P);
        const bool moved = ok && LI(IL_END, m) > LI(IL_FIRST, m);
        for (int k = 0; k < 3; ++k) {
            const double est = LD(L_EST + k, m);
            if (moved) {
                const double x = LD(L_X + k, m);
                LD(L_TRIAL + k, m) = est + x;
                acc += x * (lambda * x + LD(L_H + 6 + k, m));
            } else {
                LD(L_TRIAL + k, m) = est;
            }
        }
    }
    const double total = block_total(acc, s_val, s_row);
    if (threadIdx.x == 0) A.scale_part[blockIdx.x] = total;
}

// OptimizationAlgorithmLevenberg::solve's decisions after a trial, by one lane; the host reads rec
__global__ void ba_judge(Args A, int max_iter) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    wc::judge(*A.ctl, A.rec, A.chi_part, A.n_chi, A.scale_part, A.n_scale, max_iter);
}

// an accepted trial becomes the estimate
__global__ __launch_bounds__(kThreads) void ba_accept(Args A) {
    const size_t gi = global_tid();
    if (gi < (size_t)A.P * 7) A.wp[(size_t)P_EST * A.P + gi] = A.wp[(size_t)P_TRIAL * A.P + gi];
    if (gi < (size_t)A.M * 3) A.wl[(size_t)L_EST * A.M + gi] = A.wl[(size_t)L_TRIAL * A.M + gi];
}

// Converter::toCvMat(SE3Quat) of every pose, every point narrowed
__global__ __launch_bounds__(kThreads) void ba_write(Args A) {
    const size_t gi = global_tid();
    if (gi < (size_t)A.P) {
        const int p = (int)gi;
        const double q[4] = {PD(P_EST, p), PD(P_EST + 1, p), PD(P_EST + 2, p), PD(P_EST + 3, p)};
        const double t[3] = {PD(P_EST + 4, p), PD(P_EST + 5, p), PD(P_EST + 6, p)};
        lm::write_T16(q, t, 1.0, A.Tcw_out + 16 * gi);
    }
    if (gi < (size_t)A.M)
        for (int k = 0; k < 3; ++k) A.Xw_out[3 * gi + k] = (float)LD(L_EST + k, (int)gi);
}

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
    if (E) ORB_LAUNCH(st, ba_check, dim3(blocks_for(E)), T, a);
    if (P + M) ORB_LAUNCH(st, ba_init, dim3(blocks_for(P > M ? P : M)), T, a);
    if (E) ORB_LAUNCH(st, ba_runs, dim3(blocks_for(E)), T, a);
    ORB_LAUNCH(st, ba_scan, dim3(1), dim3(64), a);
    if (E && P) ORB_LAUNCH(st, ba_lists, dim3(blocks_for(P, kThreads / 64)), T, a);
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
            ORB_LAUNCH(st, ba_edges<true>, dim3(blocks_for(E)), T, a);
            ORB_LAUNCH(st, ba_vertex_sums, dim3(blocks_for(P * 27 + M * 9)), T, a, it == 0 ? 1 : 0);
            ORB_LAUNCH(st, ba_begin, dim3(1), dim3(64), a, it == 0 ? 1 : 0);
            iterations = it + 1;
            for (int trial = 0; trial < lm::kMaxTrials; ++trial) {
                ORB_LAUNCH(st, ba_point_inverse, dim3(blocks_for(M)), T, a);
                ORB_LAUNCH(st, ba_edge_bd, dim3(blocks_for(E)), T, a);
                if (nf) {
                    ORB_LAUNCH(st, ba_schur, dim3(blocks_for((size_t)nf * nf * 36 + n)), T, a);
                    ORB_HIP(orbgpu::chol::enqueue_solve(view, n, st));
                }
                ORB_LAUNCH(st, ba_point_x, dim3(blocks_for(M)), T, a);
                ORB_LAUNCH(st, ba_trial, dim3(blocks_for(P + M)), T, a);
                ORB_LAUNCH(st, ba_edges<false>, dim3(blocks_for(E)), T, a);
                ORB_LAUNCH(st, ba_judge, dim3(1), dim3(64), a, n_iterations);
                ORB_HIP(hipStreamSynchronize(st));
                if (rec->accepted) ORB_LAUNCH(st, ba_accept, dim3(blocks_for(P * 7 > M * 3 ? P * 7 : M * 3)), T, a);
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
    if (P + M) ORB_LAUNCH(st, ba_write, dim3(blocks_for(P > M ? P : M)), T, a);
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
