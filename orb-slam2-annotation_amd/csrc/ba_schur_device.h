// ba_schur_device.h -- the per-item arithmetic of a bundle adjustment's Schur
// step, written for localba.hip (one workgroup per job, strided loops in one
// kernel) and for globalba.hip (one lane per item, one launch per phase), which
// so far takes the field offsets from here and keeps the same text in its own
// kernels: the
// workspace's field offsets, a view of it, and per edge, pose and point the
// build of the quadratic form (core/base_binary_edge.hpp:43-120, the edges are
// projection_edge.h's), Dinv and B Dinv, the right-hand side of the reduced
// system, the back-substitution and oplus (core/block_solver.hpp:355-487,
// 565-610).  Each function is one item's work: no loop over items, no barrier.
// The assembly of S, its solve, the structure builds and computeLambdaInit's
// maximum stay with each file.
//
// `active` is a callable bool(int edge): localba.hip skips its level-1 edges
// with it; a problem without levels passes a constant true.  A skipped edge
// leaves the order of every sum's other terms as it is.
#pragma once

#include <hip/hip_runtime.h>

#include "projection_edge.h"
#include "se3_device.h"

namespace orbgpu {
namespace ba {

// doubles per pose, point and edge in the workspace, and where each field starts
constexpr int P_EST = 0, P_TRIAL = 7, P_H = 14, kPoseD = 41;                                   // q t | q t | H 21, b 6
constexpr int L_EST = 0, L_TRIAL = 3, L_H = 6, L_DINV = 15, L_V = 21, L_X = 24, kPointD = 27;  // H 6, b 3
constexpr int E_JP = 0, E_JL = 18, E_W = 27, E_OMR = 28, E_B = 31, E_BD = 49;
// ints per pose and point
constexpr int IP_HIDX = 0, IP_HLIST = 1, IP_START = 2, IP_COUNT = 3, IP_FREE = 4, kPoseI = 5;
constexpr int IL_FIRST = 0, IL_END = 1;

// a problem's slices of the workspace (structure of arrays: field f of pose p is wp[f * TP + p])
// and of the caller's arrays, indexed by the problem's own pose, point and edge numbers
struct View {
    double *wp, *wl, *we;
    int *ip, *il;
    int* list;  // the pose-major edge list: pose p's edges are list[IP_START .. + IP_COUNT), ascending
    int TP, TM, TE;  // the strides: the numbers of poses, points and edges the workspace was laid out for
    const int *edge_pose, *edge_point;
    const float *cam, *obs, *inv_sigma2;

    __device__ __forceinline__ double& PD(int f, int p) const { return wp[(size_t)f * TP + p]; }
    __device__ __forceinline__ double& LD(int f, int m) const { return wl[(size_t)f * TM + m]; }
    __device__ __forceinline__ double& ED(int f, int e) const { return we[(size_t)f * TE + e]; }
    __device__ __forceinline__ int& PI(int f, int p) const { return ip[(size_t)f * TP + p]; }
    __device__ __forceinline__ int& LI(int f, int m) const { return il[(size_t)f * TM + m]; }
};

// ------------------------------------------------------------------ per edge

// what computeError leaves of an edge
struct EdgeAt {
    double q[4], x, y, z, invz, e[3], w, chi2;
    bool stereo;
    proj_edge::Cam cam;
};

// computeError of edge i at the estimates in field est_p / est_l
__device__ __forceinline__ void edge_error(const View& V, int i, int est_p, int est_l, EdgeAt& g) {
    const int p = V.edge_pose[i], m = V.edge_point[i];
    double t[3];
    for (int k = 0; k < 4; ++k) g.q[k] = V.PD(est_p + k, p);
    for (int k = 0; k < 3; ++k) t[k] = V.PD(est_p + 4 + k, p);
    const double X[3] = {V.LD(est_l, m), V.LD(est_l + 1, m), V.LD(est_l + 2, m)};
    g.cam = proj_edge::load_cam(V.cam + 5 * (size_t)p);
    const float* ob = V.obs + 3 * (size_t)i;
    const float obs[3] = {ob[0], ob[1], ob[2]};
    g.w = (double)V.inv_sigma2[i];
    g.stereo = obs[2] >= 0.0f;
    g.chi2 = proj_edge::project_error(g.q, t, X, g.cam, obs, g.w, g.x, g.y, g.z, g.invz, g.e);
}

__device__ __forceinline__ double robustify(const EdgeAt& g, bool robust, const proj_edge::HuberConst& hc,
                                            double& rho1) {
    double rho0 = g.chi2;
    rho1 = 1.0;
    if (robust)
        lm::huber(g.chi2, g.stereo ? hc.delta_stereo : hc.delta_mono, g.stereo ? hc.dsqr_stereo : hc.dsqr_mono, rho0,
                  rho1);
    return rho0;
}

// computeActiveErrors of edge i at the trial (or any) fields: its robust chi2, and chi2 itself
__device__ __forceinline__ double edge_chi(const View& V, int i, int est_p, int est_l, bool robust,
                                           const proj_edge::HuberConst& hc, double& chi2) {
    EdgeAt g;
    edge_error(V, i, est_p, est_l, g);
    chi2 = g.chi2;
    double rho1;
    return robustify(g, robust, hc, rho1);
}

// edge_chi, then linearizeOplus and the edge's terms of buildSystem: W = rho1 w, rho1 (-(w e)),
// the two Jacobians and B = Jp^T W Jl
__device__ __forceinline__ double edge_build(const View& V, int i, int est_p, int est_l, bool robust,
                                             const proj_edge::HuberConst& hc, double& chi2) {
    EdgeAt g;
    edge_error(V, i, est_p, est_l, g);
    chi2 = g.chi2;
    double rho1;
    const double rho0 = robustify(g, robust, hc, rho1);
    double R[3][3], Jl[3][3], Jp[3][6];
    se3::quat_to_R(g.q, R);
    proj_edge::linearize_xyz_se3(g.x, g.y, g.z, R, g.cam, g.stereo, Jp, Jl);
    const double Wt = rho1 * g.w;
    V.ED(E_W, i) = Wt;
    for (int r = 0; r < 3; ++r) {
        V.ED(E_OMR + r, i) = rho1 * (-(g.w * g.e[r]));
        for (int k = 0; k < 6; ++k) V.ED(E_JP + 6 * r + k, i) = Jp[r][k];
        for (int k = 0; k < 3; ++k) V.ED(E_JL + 3 * r + k, i) = Jl[r][k];
    }
    for (int a = 0; a < 6; ++a)
        for (int col = 0; col < 3; ++col)
            V.ED(E_B + 3 * a + col, i) = ((Wt * Jp[0][a]) * Jl[0][col] + (Wt * Jp[1][a]) * Jl[1][col]) +
                                         (Wt * Jp[2][a]) * Jl[2][col];
    return rho0;
}

// Dinv (row-major, symmetric) of point m from its six stored entries
__device__ __forceinline__ void load_dinv(const View& V, int m, double (&D)[3][3]) {
    D[0][0] = V.LD(L_DINV, m), D[0][1] = V.LD(L_DINV + 1, m), D[0][2] = V.LD(L_DINV + 2, m);
    D[1][1] = V.LD(L_DINV + 3, m), D[1][2] = V.LD(L_DINV + 4, m), D[2][2] = V.LD(L_DINV + 5, m);
    D[1][0] = D[0][1], D[2][0] = D[0][2], D[2][1] = D[1][2];
}

// B Dinv of edge i (an edge that has a B: active, its pose free)
__device__ __forceinline__ void edge_bd(const View& V, int i) {
    double D[3][3];
    load_dinv(V, V.edge_point[i], D);
    for (int a = 0; a < 6; ++a) {
        const double b0 = V.ED(E_B + 3 * a, i), b1 = V.ED(E_B + 3 * a + 1, i), b2 = V.ED(E_B + 3 * a + 2, i);
        for (int k = 0; k < 3; ++k) V.ED(E_BD + 3 * a + k, i) = (b0 * D[0][k] + b1 * D[1][k]) + b2 * D[2][k];
    }
}

// ------------------------------------------------------------------ per vertex entry: buildSystem

// entry v of free pose p's 21 + 6 (the upper triangle of its block, then its right-hand side) over
// the pose's active edges ascending, for field P_H + v; diagonal: v is an entry H_jj
template <class Active>
__device__ __forceinline__ double pose_entry(const View& V, int p, int v, Active&& active, bool& diagonal) {
    const int start = V.PI(IP_START, p), count = V.PI(IP_COUNT, p);
    double acc = 0.0;
    diagonal = false;
    if (v < 21) {
        int j, k;
        lm::upper_jk<6>(v, j, k);
        for (int s = 0; s < count; ++s) {
            const int e = V.list[start + s];
            if (!active(e)) continue;
            const double Wt = V.ED(E_W, e);
            acc += ((Wt * V.ED(E_JP + j, e)) * V.ED(E_JP + k, e) + (Wt * V.ED(E_JP + 6 + j, e)) * V.ED(E_JP + 6 + k, e)) +
                   (Wt * V.ED(E_JP + 12 + j, e)) * V.ED(E_JP + 12 + k, e);
        }
        diagonal = j == k;
    } else {
        const int j = v - 21;
        for (int s = 0; s < count; ++s) {
            const int e = V.list[start + s];
            if (!active(e)) continue;
            acc += (V.ED(E_JP + j, e) * V.ED(E_OMR, e) + V.ED(E_JP + 6 + j, e) * V.ED(E_OMR + 1, e)) +
                   V.ED(E_JP + 12 + j, e) * V.ED(E_OMR + 2, e);
        }
    }
    return acc;
}

// entry v of active point m's 6 + 3 over the active edges of the point's run, for field L_H + v
template <class Active>
__device__ __forceinline__ double point_entry(const View& V, int m, int v, Active&& active, bool& diagonal) {
    const int first = V.LI(IL_FIRST, m), end = V.LI(IL_END, m);
    double acc = 0.0;
    diagonal = false;
    if (v < 6) {
        int j, k;
        lm::upper_jk<3>(v, j, k);
        for (int e = first; e < end; ++e) {
            if (!active(e)) continue;
            const double Wt = V.ED(E_W, e);
            acc += ((Wt * V.ED(E_JL + j, e)) * V.ED(E_JL + k, e) + (Wt * V.ED(E_JL + 3 + j, e)) * V.ED(E_JL + 3 + k, e)) +
                   (Wt * V.ED(E_JL + 6 + j, e)) * V.ED(E_JL + 6 + k, e);
        }
        diagonal = j == k;
    } else {
        const int j = v - 6;
        for (int e = first; e < end; ++e) {
            if (!active(e)) continue;
            acc += (V.ED(E_JL + j, e) * V.ED(E_OMR, e) + V.ED(E_JL + 3 + j, e) * V.ED(E_OMR + 1, e)) +
                   V.ED(E_JL + 6 + j, e) * V.ED(E_OMR + 2, e);
        }
    }
    return acc;
}

// ------------------------------------------------------------------ per vertex: BlockSolver::solve

// Dinv = (Hll + lambda I)^-1 of active point m from cofactors, and Dinv b_l
__device__ __forceinline__ void point_inverse(const View& V, int m, double lambda) {
    const double a = V.LD(L_H, m) + lambda, b = V.LD(L_H + 1, m), cc = V.LD(L_H + 2, m);
    const double d = V.LD(L_H + 3, m) + lambda, e = V.LD(L_H + 4, m), f = V.LD(L_H + 5, m) + lambda;
    const double c00 = d * f - e * e, c01 = cc * e - b * f, c02 = b * e - cc * d;
    const double c11 = a * f - cc * cc, c12 = b * cc - a * e, c22 = a * d - b * b;
    const double inv = 1.0 / ((a * c00 + b * c01) + cc * c02);
    const double D[3][3] = {{c00 * inv, c01 * inv, c02 * inv},
                            {c01 * inv, c11 * inv, c12 * inv},
                            {c02 * inv, c12 * inv, c22 * inv}};
    V.LD(L_DINV, m) = D[0][0], V.LD(L_DINV + 1, m) = D[0][1], V.LD(L_DINV + 2, m) = D[0][2];
    V.LD(L_DINV + 3, m) = D[1][1], V.LD(L_DINV + 4, m) = D[1][2], V.LD(L_DINV + 5, m) = D[2][2];
    const double b0 = V.LD(L_H + 6, m), b1 = V.LD(L_H + 7, m), b2 = V.LD(L_H + 8, m);
    for (int k = 0; k < 3; ++k) V.LD(L_V + k, m) = (D[k][0] * b0 + D[k][1] * b1) + D[k][2] * b2;
}

// entry j of b_schur = b_p - sum B (Dinv b_l) of the ia-th free pose
template <class Active>
__device__ __forceinline__ double b_schur_entry(const View& V, int ia, int j, Active&& active) {
    const int pa = V.PI(IP_HLIST, ia);
    const int start = V.PI(IP_START, pa), count = V.PI(IP_COUNT, pa);
    double coef = 0.0;
    for (int k = 0; k < count; ++k) {
        const int e = V.list[start + k];
        if (!active(e)) continue;
        const int m = V.edge_point[e];
        coef += (V.ED(E_B + 3 * j, e) * V.LD(L_V, m) + V.ED(E_B + 3 * j + 1, e) * V.LD(L_V + 1, m)) +
                V.ED(E_B + 3 * j + 2, e) * V.LD(L_V + 2, m);
    }
    return V.PD(P_H + 21 + j, pa) - coef;
}

// x_l = Dinv (b_l - B^T x_p) of active point m, x_p the reduced system's solution; zero after a
// failed solve
template <class Active>
__device__ __forceinline__ void point_x(const View& V, int m, const double* x_p, bool ok, Active&& active) {
    if (!ok) {
        for (int k = 0; k < 3; ++k) V.LD(L_X + k, m) = 0.0;
        return;
    }
    double t[3] = {V.LD(L_H + 6, m), V.LD(L_H + 7, m), V.LD(L_H + 8, m)};
    const int end = V.LI(IL_END, m);
    for (int e = V.LI(IL_FIRST, m); e < end; ++e) {
        const int p = V.edge_pose[e];
        if (!active(e) || !V.PI(IP_FREE, p)) continue;
        const double* xp = x_p + 6 * (size_t)V.PI(IP_HIDX, p);
        for (int k = 0; k < 3; ++k) {
            double dot = V.ED(E_B + k, e) * xp[0];
            for (int a = 1; a < 6; ++a) dot = dot + V.ED(E_B + 3 * a + k, e) * xp[a];
            t[k] -= dot;
        }
    }
    double D[3][3];
    load_dinv(V, m, D);
    for (int k = 0; k < 3; ++k) V.LD(L_X + k, m) = (D[k][0] * t[0] + D[k][1] * t[1]) + D[k][2] * t[2];
}

// ------------------------------------------------------------------ per vertex: oplus

// pose p's trial = exp(x) * estimate; x null: the pose does not move
__device__ __forceinline__ void pose_oplus(const View& V, int p, const double* xp) {
    double q[4], t[3];
    for (int k = 0; k < 4; ++k) q[k] = V.PD(P_EST + k, p);
    for (int k = 0; k < 3; ++k) t[k] = V.PD(P_EST + 4 + k, p);
    if (xp) {
        const double x[6] = {xp[0], xp[1], xp[2], xp[3], xp[4], xp[5]};
        double oq[4], ot[3];
        se3::se3_exp_times(q, t, x, oq, ot);
        for (int k = 0; k < 4; ++k) q[k] = oq[k];
        for (int k = 0; k < 3; ++k) t[k] = ot[k];
    }
    for (int k = 0; k < 4; ++k) V.PD(P_TRIAL + k, p) = q[k];
    for (int k = 0; k < 3; ++k) V.PD(P_TRIAL + 4 + k, p) = t[k];
}

// point m's trial = estimate + x_l when it moved
__device__ __forceinline__ void point_oplus(const View& V, int m, bool moved) {
    for (int k = 0; k < 3; ++k)
        V.LD(L_TRIAL + k, m) = moved ? V.LD(L_EST + k, m) + V.LD(L_X + k, m) : V.LD(L_EST + k, m);
}

}  // namespace ba
}  // namespace orbgpu
