// poseopt.hip -- Optimizer::PoseOptimization (src/Optimizer.cpp:291-513) for a
// batch of frames (include/orbgpu_poseopt.h): the motion-only refinement of one
// 6-DoF pose against its MapPoint observations, with g2o's Levenberg-Marquardt
// (core/optimization_algorithm_levenberg.cpp:61-189), the unary edges'
// quadratic form (core/base_unary_edge.hpp:43-72), Huber
// (core/robust_kernel_impl.cpp:64-91), the two OnlyPose edges
// (types/types_six_dof_expmap.cpp:285-385) and SE3Quat (types/se3quat.h).
// tests/poseopt_ref.py is the same arithmetic, expression for expression.
//
// One workgroup per job, one launch for the whole optimisation.  Edge i of a
// job belongs to lane i % T for the whole call: the lane reads it (from LDS
// when the job has at most kCap edges, else from HBM/L2), keeps its flag and
// adds its terms to 28 private doubles -- the 21 upper entries of H, b and the
// robust chi2.  One "pass" evaluates every active edge at the trial estimate
// and reduces the 28 sums in a fixed order: DPP row sums (group_sum.h), one
// LDS row per 16 lanes, then lanes 0..27 add the rows in order.  No
// floating-point atomics: a job's bits do not depend on its neighbours, its
// block index or the call.
//
// The passes of a round are one flat loop.  After each pass lane 0 advances the
// LM state machine in LDS (accept / reject, lambda, the stop rules, the next
// 6x6 solve and exp(x) * estimate) and leaves `done` there; every lane reads
// that word after the barrier, so no lane ever decides from a sum of its own.
// The system (H, b) is built in the same pass that gives a trial its chi2: an
// accepted trial's system is the next iteration's, a rejected trial keeps the
// old one, and neither is recomputed (the values would be the same bits).  The
// loop bound, 1 + 10 x 10 passes, is the reference's 10 iterations of 10
// trials; the kernel ends on any input.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/orbgpu_poseopt.h"
#include "group_sum.h"
#include "host_common.h"
#include "host_ctx.h"

namespace {

constexpr int kCap = 1536;  // edges of a job kept in LDS (7 floats and a flag byte each)
constexpr int kVals = 28;   // H (21), b (6), robust chi2
constexpr int kMaxPasses = 101;
// Workgroup size, fixed at build time.  256 is what the A/B chose; a variant
// library for the A/B is built with  make BUILD=build_t64 LIB=liborbgpu_t64.so EXTRA=-DPOSEOPT_THREADS=64
#ifndef POSEOPT_THREADS
#define POSEOPT_THREADS 256
#endif
constexpr int kThreads = POSEOPT_THREADS;
static_assert(kThreads == 64 || kThreads == 128 || kThreads == 256, "whole waves, at most 16 rows of 16 lanes");

struct Se3 {
    double q[4];  // x, y, z, w
    double t[3];
};

// (float)sqrt(5.991), (float)sqrt(7.815) and their float squares (Huber's dsqr), from the host
struct HuberConst {
    double delta_mono, delta_stereo, dsqr_mono, dsqr_stereo;
};

enum { kPhaseInit = 0, kPhaseTrial = 1 };

// the job's state in LDS; written by lane 0 between barriers, read by all
struct Ctl {
    double tot[kVals];       // the last pass' sums
    double H[21], b[6], chi; // system and robust chi2 at `est`
    Se3 est0, est, trial;
    double x[6];
    double lambda, ni, ini_chi;
    double R[9];             // scratch of quat_from_R (indexed at run time)
    double qs[4];
    int n, offset, valid, rounds;
    int phase, ok, iter, qmax, stop_bad, rejected, done, n_bad;
    float fx, fy, cx, cy, bf;
};

// ------------------------------------------------------------------ SE3Quat (lane 0)

// Eigen: Quaterniond(Matrix3d) of c.R into c.qs
__device__ void quat_from_R(Ctl& c) {
    double* R = c.R;
    double* q = c.qs;
    double t = (R[0] + R[4]) + R[8];
    if (t > 0) {
        t = __dsqrt_rn(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = __dsqrt_rn(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
}

// SE3Quat::normalizeRotation
__device__ inline void quat_normalize(double (&q)[4]) {
    if (q[3] < 0) {
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    }
    const double n = __dsqrt_rn(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}

// Eigen's Quaternion::_transformVector
__device__ __forceinline__ void quat_rotate(const double (&q)[4], double v0, double v1, double v2, double& r0,
                                            double& r1, double& r2) {
    double ux = q[1] * v2 - q[2] * v1;
    double uy = q[2] * v0 - q[0] * v2;
    double uz = q[0] * v1 - q[1] * v0;
    ux = ux + ux, uy = uy + uy, uz = uz + uz;
    r0 = (v0 + q[3] * ux) + (q[1] * uz - q[2] * uy);
    r1 = (v1 + q[3] * uy) + (q[2] * ux - q[0] * uz);
    r2 = (v2 + q[3] * uz) + (q[0] * uy - q[1] * ux);
}

// SE3Quat::exp(x) * est  (se3quat.h:223-257, 104-110)
__device__ void se3_exp_times(Ctl& c, const double (&x)[6], const Se3& est, Se3& out) {
    const double om0 = x[0], om1 = x[1], om2 = x[2];
    const double theta = __dsqrt_rn((om0 * om0 + om1 * om1) + om2 * om2);
    const double O[3][3] = {{0.0, -om2, om1}, {om2, 0.0, -om0}, {-om1, om0, 0.0}};
    double O2[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double r = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
                c.R[3 * i + j] = r;
                V[i][j] = r;
            }
    } else {
        const double sn = sin(theta), cs = cos(theta);
        const double a = sn / theta;
        const double b = (1.0 - cs) / (theta * theta);
        const double d = (theta - sn) / ((theta * theta) * theta);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double id = i == j ? 1.0 : 0.0;
                c.R[3 * i + j] = (id + a * O[i][j]) + b * O2[i][j];
                V[i][j] = (id + b * O[i][j]) + d * O2[i][j];
            }
    }
    double te[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) te[i] = (V[i][0] * x[3] + V[i][1] * x[4]) + V[i][2] * x[5];
    quat_from_R(c);
    double a[4] = {c.qs[0], c.qs[1], c.qs[2], c.qs[3]};
    quat_normalize(a);
    // SE3Quat::operator*: t = ta + qa * tb, q = qa * qb, normalised
    double r0, r1, r2;
    quat_rotate(a, est.t[0], est.t[1], est.t[2], r0, r1, r2);
    const double* bq = est.q;
    double q[4] = {((a[3] * bq[0] + a[0] * bq[3]) + a[1] * bq[2]) - a[2] * bq[1],
                   ((a[3] * bq[1] + a[1] * bq[3]) + a[2] * bq[0]) - a[0] * bq[2],
                   ((a[3] * bq[2] + a[2] * bq[3]) + a[0] * bq[1]) - a[1] * bq[0],
                   ((a[3] * bq[3] - a[0] * bq[0]) - a[1] * bq[1]) - a[2] * bq[2]};
    quat_normalize(q);
    for (int i = 0; i < 4; ++i) out.q[i] = q[i];
    out.t[0] = te[0] + r0;
    out.t[1] = te[1] + r1;
    out.t[2] = te[2] + r2;
}

// index of H(j, k), j <= k, among the 21 upper entries (row by row)
__host__ __device__ constexpr int upper_index(int j, int k) { return j * 6 - j * (j - 1) / 2 + (k - j); }

// (H + lambda I) x = b by Cholesky; false when a pivot is not positive
__device__ bool solve6(const Ctl& c, double lambda, double (&x)[6]) {
    double L[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = c.H[upper_index(j, j)] + lambda;
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0)) return false;
        L[j][j] = __dsqrt_rn(s);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double r = c.H[upper_index(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) r -= L[i][k] * L[j][k];
            L[i][j] = r / L[j][j];
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = c.b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

// the next trial: solve at the current lambda, trial = exp(x) * est (a failed
// solve: x = 0, trial = est)
__device__ void next_trial(Ctl& c) {
    double x[6];
    const bool ok = solve6(c, c.lambda, x);
    if (ok) {
        se3_exp_times(c, x, c.est, c.trial);
    } else {
        for (int i = 0; i < 6; ++i) x[i] = 0.0;
        c.trial = c.est;
    }
    for (int i = 0; i < 6; ++i) c.x[i] = x[i];
    c.ok = ok ? 1 : 0;
}

__device__ void begin_iteration(Ctl& c) {
    c.iter += 1;
    c.ini_chi = c.chi;
    c.qmax = 0;
    next_trial(c);
}

// OptimizationAlgorithmLevenberg::solve, one pass at a time: c.tot is the
// system and robust chi2 at c.trial
__device__ void lm_step(Ctl& c) {
    if (c.phase == kPhaseInit) {
        for (int i = 0; i < 21; ++i) c.H[i] = c.tot[i];
        for (int i = 0; i < 6; ++i) c.b[i] = c.tot[21 + i];
        c.chi = c.tot[27];
        double max_diag = 0.0;
        for (int j = 0; j < 6; ++j) {  // std::max(fabs(h), maxDiagonal)
            const double a = fabs(c.H[upper_index(j, j)]);
            max_diag = a < max_diag ? max_diag : a;
        }
        c.lambda = 1e-5 * max_diag;
        c.ni = 2.0;
        c.stop_bad = 0;
        c.phase = kPhaseTrial;
        begin_iteration(c);
        return;
    }
    const double tmp_chi = c.ok ? c.tot[27] : DBL_MAX;
    double scale = 0.0;
    for (int j = 0; j < 6; ++j) scale += c.x[j] * (c.lambda * c.x[j] + c.b[j]);
    scale += 1e-3;
    const double rho = (c.chi - tmp_chi) / scale;
    if (rho > 0 && isfinite(tmp_chi)) {
        const double t3 = 2.0 * rho - 1.0;
        double alpha = 1.0 - (t3 * t3) * t3;
        alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
        c.lambda *= (1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0);
        c.ni = 2.0;
        c.chi = tmp_chi;
        c.est = c.trial;
        for (int i = 0; i < 21; ++i) c.H[i] = c.tot[i];
        for (int i = 0; i < 6; ++i) c.b[i] = c.tot[21 + i];
    } else {
        c.lambda *= c.ni;
        c.ni *= 2.0;
        c.rejected += 1;
    }
    c.qmax += 1;
    if (rho < 0 && c.qmax < 10) {
        next_trial(c);
        return;
    }
    if (c.qmax == 10 || rho == 0) {
        c.done = 1;
        return;
    }
    if ((c.ini_chi - c.chi) * 1e3 < c.ini_chi)
        c.stop_bad += 1;
    else
        c.stop_bad = 0;
    if (c.stop_bad >= 3 || c.iter >= 10) {
        c.done = 1;
        return;
    }
    begin_iteration(c);
}

// ------------------------------------------------------------------ the edges (every lane)

struct Edge {
    float X[3], u, v, ur, w;
};

struct Cam {
    double fx, fy, cx, cy, bf;
};

// computeError at (q, t): camera-frame point, error, chi2 = e . (w e).  invz = 1.0 / z is taken
// once, ahead of the branch: the stereo projection rounds it to float, linearizeOplus uses it as it is.
__device__ __forceinline__ double edge_error(const Se3& s, const Edge& ed, const Cam& cam, double& x, double& y,
                                             double& z, double& invz, double (&e)[3]) {
    double r0, r1, r2;
    quat_rotate(s.q, (double)ed.X[0], (double)ed.X[1], (double)ed.X[2], r0, r1, r2);
    x = r0 + s.t[0];
    y = r1 + s.t[1];
    z = r2 + s.t[2];
    invz = 1.0 / z;
    const double w = (double)ed.w;
    if (ed.ur >= 0.0f) {
        // const float invz = 1.0f / trans_xyz[2]: trans_xyz is a Vector3d, so the quotient is taken
        // in double and rounded to float once
        const double invzf = (double)(float)invz;
        const double us = (x * invzf) * cam.fx + cam.cx;
        const double vs = (y * invzf) * cam.fy + cam.cy;
        const double rs = us - cam.bf * invzf;
        e[0] = (double)ed.u - us;
        e[1] = (double)ed.v - vs;
        e[2] = (double)ed.ur - rs;
        return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
    }
    e[0] = (double)ed.u - ((x / z) * cam.fx + cam.cx);
    e[1] = (double)ed.v - ((y / z) * cam.fy + cam.cy);
    e[2] = 0.0;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// structural zeros of the Jacobian rows (columns 4, 3, 4): their products are skipped
__host__ __device__ constexpr bool non_zero(int r, int j) { return r == 1 ? j != 3 : j != 4; }

// H += J^T (rho1 w) J, b_acc += rho1 J^T (w e) over Rows residual rows
template <int Rows>
__device__ __forceinline__ void accumulate(double (&acc)[kVals], const double (&J)[3][6], double W, double rho1,
                                           const double (&we)[3]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int k = j; k < 6; ++k) {
            double c = 0.0;
            bool have = false;
#pragma unroll
            for (int r = 0; r < Rows; ++r) {
                if (non_zero(r, j) && non_zero(r, k)) {
                    const double term = (W * J[r][j]) * J[r][k];
                    c = have ? c + term : term;
                    have = true;
                }
            }
            if (have) acc[upper_index(j, k)] += c;
        }
        double c = 0.0;
        bool have = false;
#pragma unroll
        for (int r = 0; r < Rows; ++r) {
            if (non_zero(r, j)) {
                const double term = J[r][j] * we[r];
                c = have ? c + term : term;
                have = true;
            }
        }
        acc[21 + j] += rho1 * c;
    }
}

template <int T>
__global__ __launch_bounds__(T) void poseopt_kernel(const orbgpu_poseopt_job* __restrict__ jobs, int total_obs,
                                                    const float* __restrict__ Xw, const float* __restrict__ obs,
                                                    const float* __restrict__ inv_sigma2,
                                                    orbgpu_poseopt_result* __restrict__ results,
                                                    uint8_t* __restrict__ outlier, HuberConst hc) {
    __shared__ Ctl ctl;
    __shared__ double s_part[T / 16][kVals];
    __shared__ float s_edge[7][kCap];
    __shared__ uint8_t s_flag[kCap];

    const int tid = threadIdx.x;
    const orbgpu_poseopt_job* job = jobs + blockIdx.x;
    if (tid == 0) {
        const int n = job->n, offset = job->offset;
        const bool valid = n >= 0 && offset >= 0 && (long long)offset + n <= (long long)total_obs;
        ctl.valid = valid ? 1 : 0;
        ctl.n = valid ? n : 0;
        ctl.offset = valid ? offset : 0;
        ctl.rounds = !valid || n < 3 ? 0 : (n < 10 ? 1 : 4);
        ctl.fx = job->fx, ctl.fy = job->fy, ctl.cx = job->cx, ctl.cy = job->cy, ctl.bf = job->bf;
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 3; ++col) ctl.R[3 * r + col] = (double)job->Tcw0[4 * r + col];
        quat_from_R(ctl);  // Converter::toSE3Quat
        double q[4] = {ctl.qs[0], ctl.qs[1], ctl.qs[2], ctl.qs[3]};
        quat_normalize(q);
        for (int i = 0; i < 4; ++i) ctl.est0.q[i] = q[i];
        for (int r = 0; r < 3; ++r) ctl.est0.t[r] = (double)job->Tcw0[4 * r + 3];
        ctl.est = ctl.est0;
        ctl.trial = ctl.est0;
        ctl.n_bad = 0;
    }
    __syncthreads();
    const int n = ctl.n;
    const size_t base = (size_t)ctl.offset;
    const bool on_chip = n <= kCap;
    const int rounds = ctl.rounds;
    const Cam cam = {(double)ctl.fx, (double)ctl.fy, (double)ctl.cx, (double)ctl.cy, (double)ctl.bf};
    uint8_t* g_flag = outlier + base;

    for (int i = tid; i < n; i += T) {
        if (on_chip) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_edge[k][i] = Xw[3 * (base + i) + k];
                s_edge[3 + k][i] = obs[3 * (base + i) + k];
            }
            s_edge[6][i] = inv_sigma2[base + i];
            s_flag[i] = 0;
        } else {
            g_flag[i] = 0;
        }
    }
    // lane i % T alone touches edge i, its LDS copy and its flag: no barrier is needed for them

    auto load_edge = [&](int i) {
        Edge ed;
        if (on_chip) {
            ed.X[0] = s_edge[0][i], ed.X[1] = s_edge[1][i], ed.X[2] = s_edge[2][i];
            ed.u = s_edge[3][i], ed.v = s_edge[4][i], ed.ur = s_edge[5][i], ed.w = s_edge[6][i];
        } else {
            const float* px = Xw + 3 * (base + i);
            const float* po = obs + 3 * (base + i);
            ed.X[0] = px[0], ed.X[1] = px[1], ed.X[2] = px[2];
            ed.u = po[0], ed.v = po[1], ed.ur = po[2], ed.w = inv_sigma2[base + i];
        }
        return ed;
    };

    int lm_iterations[4] = {0, 0, 0, 0}, lm_rejected[4] = {0, 0, 0, 0};  // lane 0's
    for (int round = 0; round < rounds; ++round) {
        if (tid == 0) {
            ctl.est = ctl.est0;  // setEstimate(toSE3Quat(pFrame->mTcw)), every round
            ctl.trial = ctl.est0;
            ctl.phase = kPhaseInit;
            ctl.iter = 0, ctl.qmax = 0, ctl.rejected = 0, ctl.done = 0, ctl.ok = 1;
            ctl.n_bad = 0;
        }
        __syncthreads();
        const bool robust = round < 3;  // the kernels are removed after round 2's classification

        for (int pass = 0; pass < kMaxPasses; ++pass) {
            const Se3 s = ctl.trial;
            double acc[kVals];
#pragma unroll
            for (int v = 0; v < kVals; ++v) acc[v] = 0.0;
            for (int i = tid; i < n; i += T) {
                if (on_chip ? s_flag[i] : g_flag[i]) continue;  // level 1
                const Edge ed = load_edge(i);
                double x, y, z, invz, e[3];
                const double chi2 = edge_error(s, ed, cam, x, y, z, invz, e);
                const bool stereo = ed.ur >= 0.0f;
                double rho0 = chi2, rho1 = 1.0;
                if (robust) {  // RobustKernelHuber::robustify
                    const double delta = stereo ? hc.delta_stereo : hc.delta_mono;
                    const double dsqr = stereo ? hc.dsqr_stereo : hc.dsqr_mono;
                    if (!(chi2 <= dsqr)) {
                        const double sq = __dsqrt_rn(chi2);
                        rho0 = (2.0 * sq) * delta - dsqr;
                        rho1 = delta / sq;
                    }
                }
                // linearizeOplus
                const double invz2 = invz * invz;
                double J[3][6];
                J[0][0] = ((x * y) * invz2) * cam.fx;
                J[0][1] = (-(1.0 + (x * x) * invz2)) * cam.fx;
                J[0][2] = (y * invz) * cam.fx;
                J[0][3] = (-invz) * cam.fx;
                J[0][4] = 0.0;
                J[0][5] = (x * invz2) * cam.fx;
                J[1][0] = (1.0 + (y * y) * invz2) * cam.fy;
                J[1][1] = (((-x) * y) * invz2) * cam.fy;
                J[1][2] = ((-x) * invz) * cam.fy;
                J[1][3] = 0.0;
                J[1][4] = (-invz) * cam.fy;
                J[1][5] = (y * invz2) * cam.fy;
                const double w = (double)ed.w;
                const double W = rho1 * w;
                const double we[3] = {w * e[0], w * e[1], w * e[2]};
                if (stereo) {
                    J[2][0] = J[0][0] - (cam.bf * y) * invz2;
                    J[2][1] = J[0][1] + (cam.bf * x) * invz2;
                    J[2][2] = J[0][2];
                    J[2][3] = J[0][3];
                    J[2][4] = 0.0;
                    J[2][5] = J[0][5] - cam.bf * invz2;
                    accumulate<3>(acc, J, W, rho1, we);
                } else {
                    accumulate<2>(acc, J, W, rho1, we);
                }
                acc[27] += rho0;
            }
            // fixed-order sum over the workgroup: 16-lane rows on DPP, rows through LDS
#pragma unroll
            for (int v = 0; v < kVals; ++v) acc[v] = orbgpu::row16_sum(acc[v]);
            if ((tid & 15) == 0) {
#pragma unroll
                for (int v = 0; v < kVals; ++v) s_part[tid >> 4][v] = acc[v];
            }
            __syncthreads();
            if (tid < kVals) {
                double sum = s_part[0][tid];
                for (int r = 1; r < T / 16; ++r) sum += s_part[r][tid];
                ctl.tot[tid] = tid >= 21 && tid < 27 ? -sum : sum;  // b -= rho1 J^T w e
            }
            __syncthreads();
            if (tid == 0) lm_step(ctl);
            __syncthreads();
            if (ctl.done) break;
        }

        // classification (Optimizer.cpp:443-500): an active edge keeps the error of the last
        // trial, accepted or not; a flagged edge is recomputed at the (restored) estimate
        {
            const Se3 s_trial = ctl.trial, s_est = ctl.est;
            int bad = 0;
            for (int i = tid; i < n; i += T) {
                const bool flagged = on_chip ? s_flag[i] : g_flag[i];
                const Edge ed = load_edge(i);
                double x, y, z, invz, e[3];
                const double chi2 = edge_error(flagged ? s_est : s_trial, ed, cam, x, y, z, invz, e);
                const bool out = (float)chi2 > (ed.ur >= 0.0f ? 7.815f : 5.991f);
                if (on_chip)
                    s_flag[i] = out;
                else
                    g_flag[i] = out;
                bad += out;
            }
            if (bad) atomicAdd(&ctl.n_bad, bad);  // integers: any order gives the same sum
        }
        __syncthreads();
        if (tid == 0) {
            lm_iterations[round] = ctl.iter;
            lm_rejected[round] = ctl.rejected;
        }
    }
    __syncthreads();

    if (on_chip && ctl.valid) {
        for (int i = tid; i < n; i += T) g_flag[i] = s_flag[i];
    }
    if (tid == 0) {
        orbgpu_poseopt_result* r = results + blockIdx.x;
        r->n_good = ctl.valid ? (rounds ? n - ctl.n_bad : 0) : -1;
        r->rounds = ctl.valid ? rounds : -1;
        for (int k = 0; k < 4; ++k) r->lm_iterations[k] = lm_iterations[k], r->lm_rejected[k] = lm_rejected[k];
        float* T16 = r->Tcw;
        if (rounds == 0) {
            for (int k = 0; k < 12; ++k) T16[k] = job->Tcw0[k];
        } else {  // Converter::toCvMat(SE3Quat): toRotationMatrix, translation
            const double x = ctl.est.q[0], y = ctl.est.q[1], z = ctl.est.q[2], w = ctl.est.q[3];
            const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
            const double twx = tx * w, twy = ty * w, twz = tz * w;
            const double txx = tx * x, txy = ty * x, txz = tz * x;
            const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
            T16[0] = (float)(1.0 - (tyy + tzz)), T16[1] = (float)(txy - twz), T16[2] = (float)(txz + twy);
            T16[4] = (float)(txy + twz), T16[5] = (float)(1.0 - (txx + tzz)), T16[6] = (float)(tyz - twx);
            T16[8] = (float)(txz - twy), T16[9] = (float)(tyz + twx), T16[10] = (float)(1.0 - (txx + tyy));
            T16[3] = (float)ctl.est.t[0], T16[7] = (float)ctl.est.t[1], T16[11] = (float)ctl.est.t[2];
        }
        T16[12] = 0.0f, T16[13] = 0.0f, T16[14] = 0.0f, T16[15] = 1.0f;
    }
}

HuberConst huber_constants() {
    const float dm = (float)std::sqrt(5.991), ds = (float)std::sqrt(7.815);  // Optimizer.cpp:331-332
    // robust_kernel_impl.h:85: float dsqr = delta * delta (delta a double)
    return {(double)dm, (double)ds, (double)(float)((double)dm * (double)dm), (double)(float)((double)ds * (double)ds)};
}

}  // namespace

extern "C" int orbgpu_pose_optimization_batch_device(int batch, const orbgpu_poseopt_job* d_jobs, int total_obs,
                                                     const float* d_Xw, const float* d_obs,
                                                     const float* d_inv_sigma2, orbgpu_poseopt_result* d_results,
                                                     uint8_t* d_outlier, void* stream) {
    if (batch < 0 || total_obs < 0) return orbgpu::fail(ORBGPU_ERR_ARG, "negative batch or total_obs");
    if (batch > 0 && (!d_jobs || !d_results)) return orbgpu::fail(ORBGPU_ERR_ARG, "null jobs or results");
    if (batch > 0 && total_obs > 0 && (!d_Xw || !d_obs || !d_inv_sigma2 || !d_outlier))
        return orbgpu::fail(ORBGPU_ERR_ARG, "null observation array");
    if (batch == 0) return ORBGPU_OK;
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HuberConst hc = huber_constants();
    hipLaunchKernelGGL(poseopt_kernel<kThreads>, dim3(batch), dim3(kThreads), 0, s, d_jobs, total_obs, d_Xw, d_obs,
                       d_inv_sigma2, d_results, d_outlier, hc);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_pose_optimization_batch(int batch, const orbgpu_poseopt_job* jobs, int total_obs,
                                              const float* Xw, const float* obs, const float* inv_sigma2,
                                              orbgpu_poseopt_result* results, uint8_t* outlier) {
    using namespace orbgpu;
    if (batch < 0 || total_obs < 0) return fail(ORBGPU_ERR_ARG, "negative batch or total_obs");
    if (batch > 0 && (!jobs || !results)) return fail(ORBGPU_ERR_ARG, "null jobs or results");
    if (batch > 0 && total_obs > 0 && (!Xw || !obs || !inv_sigma2 || !outlier))
        return fail(ORBGPU_ERR_ARG, "null observation array");
    for (int b = 0; b < batch; ++b) {
        const orbgpu_poseopt_job& j = jobs[b];
        if (j.n < 0 || j.offset < 0 || (long long)j.offset + j.n > (long long)total_obs)
            return fail(ORBGPU_ERR_ARG, "job " + std::to_string(b) + " is out of the array bounds");
    }
    if (batch == 0) return ORBGPU_OK;
    if (total_obs == 0) {  // every job has n == 0: nothing to optimise, nothing to launch
        for (int b = 0; b < batch; ++b) {
            std::memset(&results[b], 0, sizeof(results[b]));
            std::memcpy(results[b].Tcw, jobs[b].Tcw0, sizeof(jobs[b].Tcw0));
            results[b].Tcw[15] = 1.0f;
        }
        return ORBGPU_OK;
    }
    int rc = check_device();
    if (rc) return rc;
    const size_t to = (size_t)total_obs;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    HostCall call(*ctx);
    const orbgpu_poseopt_job* dj;
    const float *dx, *dob, *dw;
    orbgpu_poseopt_result* dr;
    uint8_t* dout;
    rc = call.run([&](HostCall& A) {
        dj = A.in(jobs, (size_t)batch);
        dx = A.in(Xw, 3 * to);
        dob = A.in(obs, 3 * to);
        dw = A.in(inv_sigma2, to);
        dout = A.inout(outlier, to);  // bytes outside every job's range keep the caller's values
        dr = A.out<orbgpu_poseopt_result>((size_t)batch);
    });
    if (rc) return rc;
    rc = orbgpu_pose_optimization_batch_device(batch, dj, total_obs, dx, dob, dw, dr, dout, ctx->stream);
    if (rc) return rc;
    call.fetch(dr, results, sizeof(*dr) * batch);
    call.fetch(dout, outlier, to);
    return call.finish();
}
