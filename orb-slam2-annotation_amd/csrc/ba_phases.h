// ba_phases.h -- the phases of a bundle adjustment spread over the whole chip,
// one launch each: the kernels globalba.hip was written with (its header says
// what each sum's order is), as templates over the argument block so that
// localba_chip.hip runs the same bodies with LocalBA's levels.  There is one
// copy of every phase; what a problem with levels adds stands behind
// `if constexpr (AT::kLevels)`, so the instantiation over Args is, instruction
// for instruction, the code globalba.hip had.
//
// With levels (LevelArgs): an edge whose level word is set is masked -- the
// build and trial passes skip it (it adds nothing to the robust chi2 and keeps
// its stored chi2), the vertex sums, B Dinv, the merge of the Schur assembly,
// b_schur and the back-substitution step over it; the pose and point lists
// themselves stay whole.  The round's active set is what ba_scan is given:
// IP_FREE per pose and an empty run for a point without a level-0 edge, both
// made by the file that owns the levels.  After a failed solve the trial edge
// pass still runs (the trial is the kept estimate then), so that every active
// edge holds the kept estimate's chi2.  Only the n_local first poses are local:
// the others are fixed, and only the local ones are written.
//
// The including file #undefs PD, LD, ED, PI and LI after its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_schur_device.h"
#include "wholechip_lm.h"

namespace orbgpu {
namespace ba_phases {

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

// the optimisation's state on the device (wholechip::CtlBase's members and computeLambdaInit's maximum);
// zeroed by the call, then written by one lane of one kernel at a time
struct Ctl {
    lm::Run run;
    unsigned long long max_bits;  // computeLambdaInit's maximum, as bits
    double first_chi;
    int bad, fail, nf, n_active;
};
static_assert(sizeof(Ctl) <= kCtlBytes, "Ctl outgrew its slot");

// what every kernel gets
struct Args {
    static constexpr bool kLevels = false;
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

// the same with LocalBA's levels
struct LevelArgs : Args {
    static constexpr bool kLevels = true;
    int n_local;       // the poses [n_local, P) are fixed whatever `fixed` holds, and not written
    int second_round;  // ba_scan: take IP_FREE as given instead of "has an edge and is not fixed"
    int* level;        // per edge: 1 masks it
    double* last_chi2; // per edge: chi2 of the last pass that evaluated it
    int* counts;       // [0] edges sent to level 1, [1] edges to erase, [2] the second round's active points
    uint8_t* erase;
};

// edge e is at level 1
template <class AT>
__device__ __forceinline__ bool masked(const AT& A, int e) {
    if constexpr (AT::kLevels)
        return A.level[e] != 0;
    else
        return false;
}

template <class AT>
__device__ __forceinline__ bool pose_fixed(const AT& A, int p) {
    if constexpr (AT::kLevels)
        return p >= A.n_local || A.fixed[p];
    else
        return A.fixed[p];
}

#define PD(f, p) A.wp[(size_t)(f) * A.P + (p)]
#define LD(f, m) A.wl[(size_t)(f) * A.M + (m)]
#define ED(f, e) A.we[(size_t)(f) * A.E + (e)]
#define PI(f, p) A.ip[(size_t)(f) * A.P + (p)]
#define LI(f, m) A.il[(size_t)(f) * A.M + (m)]

// ------------------------------------------------------------------ once per call: check and structure

// an edge index out of range or edge_point decreasing: nothing else may index with these arrays
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_check(AT A) {
    const size_t i = global_tid();
    if (i >= (size_t)A.E) return;
    if constexpr (AT::kLevels) A.level[i] = 0, A.last_chi2[i] = 0.0;  // every edge at level 0, none evaluated
    const int p = A.edge_pose[i], m = A.edge_point[i];
    if (p < 0 || p >= A.P || m < 0 || m >= A.M || (i > 0 && A.edge_point[i - 1] > m)) A.ctl->bad = 1;
}

// Converter::toSE3Quat of every pose, every point widened; the counters cleared
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_init(AT A) {
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
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_runs(AT A) {
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
template <class AT>
__global__ void ba_scan(AT A) {
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
        int is_free;
        if constexpr (AT::kLevels)  // the second round's IP_FREE is given: a level-0 edge touches the pose
            is_free = A.second_round ? PI(IP_FREE, p) : (count > 0 && !pose_fixed(A, p));
        else
            is_free = count > 0 && !A.fixed[p];
        PI(IP_FREE, p) = is_free;
        PI(IP_HIDX, p) = -1;
        if (is_free) PI(IP_HIDX, p) = nf, PI(IP_HLIST, nf) = p, ++nf;
    }
    if constexpr (AT::kLevels) {
        if (A.second_round) {  // optimize() again: lambda, ni and the stop counter afresh
            lm::run_start(A.ctl->run);
            A.ctl->max_bits = 0, A.ctl->first_chi = 0.0, A.ctl->n_active = A.counts[2];
        }
    }
    A.ctl->nf = nf;
    rec->nf = nf, rec->n_active = A.ctl->n_active;
    __threadfence_system();
}

// the pose-major edge list, ascending: one wave per pose scans the edges 64 at a time
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_lists(AT A) {
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
template <class AT>
__device__ inline double edge_error(const AT& A, int i, int est_p, int est_l, double& x, double& y, double& z,
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
template <class AT, bool kBuild>
__global__ __launch_bounds__(kThreads) void ba_edges(AT A) {
    __shared__ double s_val[kThreads];
    __shared__ double s_row[16];
    if constexpr (!AT::kLevels) {  // with levels the pass runs on: the trial is the kept estimate
        if (!kBuild && A.ctl->fail) return;
    }
    const size_t gi = global_tid();
    double rho0 = 0.0;
    if (gi < (size_t)A.E && !masked(A, (int)gi)) {
        const int i = (int)gi;
        double x, y, z, e[3], q[4], w;
        bool stereo;
        const float* cam;
        const double chi2 = edge_error(A, i, kBuild ? P_EST : P_TRIAL, kBuild ? L_EST : L_TRIAL, x, y, z, e, q, w, stereo,
                                       cam);
        if constexpr (AT::kLevels) A.last_chi2[i] = chi2;
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

template <class AT>
__device__ inline void note_diagonal(const AT& A, double h) {
    atomicMax(&A.ctl->max_bits, (unsigned long long)__double_as_longlong(fabs(h)));
}

// the diagonal blocks and right-hand sides of buildSystem: one lane per entry, 27 per pose, then 9
// per point; in the first iteration the diagonal entries enter computeLambdaInit's maximum
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_vertex_sums(AT A, int first) {
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
                if constexpr (AT::kLevels) if (masked(A, e)) continue;
                const double Wt = ED(E_W, e);
                acc += ((Wt * ED(E_JP + j, e)) * ED(E_JP + k, e) + (Wt * ED(E_JP + 6 + j, e)) * ED(E_JP + 6 + k, e)) +
                       (Wt * ED(E_JP + 12 + j, e)) * ED(E_JP + 12 + k, e);
            }
            if (first && j == k) note_diagonal(A, acc);
        } else {
            const int j = v - 21;
            for (int s = 0; s < count; ++s) {
                const int e = A.ie[start + s];
                if constexpr (AT::kLevels) if (masked(A, e)) continue;
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
            if constexpr (AT::kLevels) if (masked(A, e)) continue;
            const double Wt = ED(E_W, e);
            acc += ((Wt * ED(E_JL + j, e)) * ED(E_JL + k, e) + (Wt * ED(E_JL + 3 + j, e)) * ED(E_JL + 3 + k, e)) +
                   (Wt * ED(E_JL + 6 + j, e)) * ED(E_JL + 6 + k, e);
        }
        if (first && j == k) note_diagonal(A, acc);
    } else {
        const int j = v - 6;
        for (int e = begin; e < end; ++e) {
            if constexpr (AT::kLevels) if (masked(A, e)) continue;
            acc += (ED(E_JL + j, e) * ED(E_OMR, e) + ED(E_JL + 3 + j, e) * ED(E_OMR + 1, e)) +
                   ED(E_JL + 6 + j, e) * ED(E_OMR + 2, e);
        }
    }
    LD(L_H + v, m) = acc;
}

// the iteration begins: the robust chi2 at the kept estimates, computeLambdaInit in the first
template <class AT>
__global__ void ba_begin(AT A, int first) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Ctl& c = *A.ctl;
    wc::begin_iteration(c, A.chi_part, A.n_chi, first, [&c](lm::Run& run) {
        lm::run_init_lambda(run, __longlong_as_double((long long)c.max_bits));
    });
}

// Dinv = (Hll + lambda I)^-1 from cofactors and Dinv b_l, one lane per point
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_point_inverse(AT A) {
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
template <class AT>
__device__ inline void load_dinv(const AT& A, int m, double (&D)[3][3]) {
    D[0][0] = LD(L_DINV, m), D[0][1] = LD(L_DINV + 1, m), D[0][2] = LD(L_DINV + 2, m);
    D[1][1] = LD(L_DINV + 3, m), D[1][2] = LD(L_DINV + 4, m), D[2][2] = LD(L_DINV + 5, m);
    D[1][0] = D[0][1], D[2][0] = D[0][2], D[2][1] = D[1][2];
}

// B Dinv of every edge that has a B (its pose is free), one lane per edge
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_edge_bd(AT A) {
    const size_t gi = global_tid();
    if (gi >= (size_t)A.E) return;
    const int i = (int)gi;
    if (!PI(IP_FREE, A.edge_pose[i]) || masked(A, i)) return;
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
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_schur(AT A) {
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
            if constexpr (AT::kLevels) if (masked(A, e)) continue;
            while (jb < cb && epoint[A.ie[sb + jb]] < m) ++jb;
            if (jb >= cb) break;
            if (epoint[A.ie[sb + jb]] != m) continue;
            const double d0 = ED(E_BD + 3 * r, e), d1 = ED(E_BD + 3 * r + 1, e), d2 = ED(E_BD + 3 * r + 2, e);
            for (int j2 = jb; j2 < cb; ++j2) {
                const int e2 = A.ie[sb + j2];
                if (epoint[e2] != m) break;
                if constexpr (AT::kLevels) if (masked(A, e2)) continue;
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
        if constexpr (AT::kLevels) if (masked(A, e)) continue;
        coef += (ED(E_B + 3 * j, e) * LD(L_V, m) + ED(E_B + 3 * j + 1, e) * LD(L_V + 1, m)) +
                ED(E_B + 3 * j + 2, e) * LD(L_V + 2, m);
    }
    A.S[n * n + wi] = PD(P_H + 21 + j, pa) - coef;
}

// ------------------------------------------------------------------ the step, the trial, the judge

// x_l = Dinv (b_l - B^T x_p), one lane per point; zero after a failed solve
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_point_x(AT A) {
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
        if (!PI(IP_FREE, p) || masked(A, e)) continue;
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
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_trial(AT A) {
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
template <class AT>
__global__ void ba_judge(AT A, int max_iter) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    wc::judge(*A.ctl, A.rec, A.chi_part, A.n_chi, A.scale_part, A.n_scale, max_iter);
}

// an accepted trial becomes the estimate
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_accept(AT A) {
    const size_t gi = global_tid();
    if (gi < (size_t)A.P * 7) A.wp[(size_t)P_EST * A.P + gi] = A.wp[(size_t)P_TRIAL * A.P + gi];
    if (gi < (size_t)A.M * 3) A.wl[(size_t)L_EST * A.M + gi] = A.wl[(size_t)L_TRIAL * A.M + gi];
}

// Converter::toCvMat(SE3Quat) of every pose, every point narrowed
template <class AT>
__global__ __launch_bounds__(kThreads) void ba_write(AT A) {
    const size_t gi = global_tid();
    size_t n_out = (size_t)A.P;
    if constexpr (AT::kLevels) n_out = (size_t)A.n_local;
    if (gi < n_out) {
        const int p = (int)gi;
        const double q[4] = {PD(P_EST, p), PD(P_EST + 1, p), PD(P_EST + 2, p), PD(P_EST + 3, p)};
        const double t[3] = {PD(P_EST + 4, p), PD(P_EST + 5, p), PD(P_EST + 6, p)};
        lm::write_T16(q, t, 1.0, A.Tcw_out + 16 * gi);
    }
    if (gi < (size_t)A.M)
        for (int k = 0; k < 3; ++k) A.Xw_out[3 * gi + k] = (float)LD(L_EST + k, (int)gi);
}

}  // namespace ba_phases
}  // namespace orbgpu
