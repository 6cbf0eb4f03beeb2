// lm_device.h -- what the one-workgroup-per-job dense optimisers (poseopt.hip,
// 6 unknowns; sim3opt.hip, 7) share: g2o's Levenberg-Marquardt
// (core/optimization_algorithm_levenberg.cpp:61-189) as a state machine that
// lane 0 advances one pass at a time, the Cholesky solve of (H + lambda I) x = b,
// Huber (core/robust_kernel_impl.cpp:64-91), the Eigen quaternion algebra and
// the Rodrigues block of SE3Quat::exp / Sim3(Vector7d), the fixed-order
// workgroup sum of the per-lane accumulators and the pose's write-out as a
// 4x4 float matrix.  tests/lm_ref.py is the same arithmetic, expression for
// expression.  Everything is indexed at compile time, so a lane keeps its
// values in registers.  A kernel adds its estimate type, its update
// exp(x) * estimate and its edges.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "group_sum.h"

namespace orbgpu {
namespace lm {

// ------------------------------------------------------------------ the solve (host and device)

__device__ inline double sqrt_rn(double v) { return __dsqrt_rn(v); }
__host__ inline double sqrt_rn(double v) { return std::sqrt(v); }

// index of H(j, k), j <= k, among the N (N + 1) / 2 upper entries (row by row)
template <int N>
__host__ __device__ constexpr int upper_index(int j, int k) {
    return j * N - j * (j - 1) / 2 + (k - j);
}
// its inverse: (j, k), j <= k, of upper entry v
template <int N>
__device__ inline void upper_jk(int v, int& j, int& k) {
    j = 0;
    while (v >= N - j) v -= N - j, ++j;
    k = j + v;
}
// index of L(i, j), j <= i, in the lower triangle (row by row)
__host__ __device__ constexpr int lower_index(int i, int j) { return i * (i + 1) / 2 + j; }

// (H + lambda I) x = b by Cholesky; false when a pivot is not positive (or NaN).  L (N (N + 1) / 2)
// and y (N) are the caller's: registers, or LDS where registers are short.
template <int N>
__host__ __device__ inline bool cholesky_solve(const double* H, const double* b, double lambda, double* x, double* L,
                                               double* y) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = H[upper_index<N>(j, j)] + lambda;
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[lower_index(j, k)] * L[lower_index(j, k)];
        if (!(s > 0)) return false;
        const double d = sqrt_rn(s);
        L[lower_index(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double r = H[upper_index<N>(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) r -= L[lower_index(i, k)] * L[lower_index(j, k)];
            L[lower_index(i, j)] = r / d;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[lower_index(i, k)] * y[k];
        y[i] = s / L[lower_index(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= L[lower_index(k, i)] * x[k];
        x[i] = s / L[lower_index(i, i)];
    }
    return true;
}

// Converter::toCvMat of (q, t, s): row-major [s R t; 0 1], R = toRotationMatrix() of q = (x, y, z, w)
__host__ __device__ inline void write_T16(const double* q, const double* t, double s, float* T16) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    T16[0] = (float)(s * (1.0 - (tyy + tzz))), T16[1] = (float)(s * (txy - twz)), T16[2] = (float)(s * (txz + twy));
    T16[4] = (float)(s * (txy + twz)), T16[5] = (float)(s * (1.0 - (txx + tzz))), T16[6] = (float)(s * (tyz - twx));
    T16[8] = (float)(s * (txz - twy)), T16[9] = (float)(s * (tyz + twx)), T16[10] = (float)(s * (1.0 - (txx + tyy)));
    T16[3] = (float)t[0], T16[7] = (float)t[1], T16[11] = (float)t[2];
    T16[12] = 0.0f, T16[13] = 0.0f, T16[14] = 0.0f, T16[15] = 1.0f;
}

// ------------------------------------------------------------------ Levenberg-Marquardt (lane 0)

constexpr double kTau = 1e-5;            // lambda_0 = kTau * max |H_jj|
constexpr double kAlphaMax = 2.0 / 3.0;  // an accepted step scales lambda by
constexpr double kAlphaMin = 1.0 / 3.0;  //   clamp(1 - (2 rho - 1)^3, kAlphaMin, kAlphaMax)
constexpr double kScaleGuard = 1e-3;     // computeScale's additive term
constexpr double kStopGain = 1e3;        // ORB-SLAM2: (ini_chi - chi) * kStopGain < ini_chi is a bad iteration
constexpr int kMaxTrials = 10;           // trials of one iteration
constexpr int kMaxBadIterations = 3;     // bad iterations in a row that end the optimisation

// what the pass now due evaluates: the system at `est` (the first of an optimisation, a later
// one) or a trial
enum Phase { kInit = 0, kRebuild = 1, kTrial = 2 };

// the optimisation's state in LDS; written by lane 0 between barriers, read by all
template <int N, class Est>
struct State {
    static constexpr int kUpper = N * (N + 1) / 2;
    static constexpr int kVals = kUpper + N + 1;  // H, b, robust chi2
    double tot[kVals];                            // the last pass' sums
    double H[kUpper], b[N], chi;                  // system and robust chi2 at `est`
    double x[N];
    Est est, trial;
    double lambda, ni, ini_chi;
    int phase, ok, iter, max_iter, qmax, stop_bad, rejected, done;
};

// initializeOptimization + optimize(max_iter) from c.est: lambda, ni and the stop counter are set
// by the first pass
template <int N, class Est>
__device__ inline void start(State<N, Est>& c, int max_iter) {
    c.trial = c.est;
    c.phase = kInit;
    c.max_iter = max_iter;
    c.iter = 0, c.qmax = 0, c.rejected = 0, c.done = 0, c.ok = 1;
}

// the next trial: solve at the current lambda, trial = oplus(x) on est (a failed solve: x = 0,
// trial = est).  oplus may change x (VertexSim3Expmap zeroes x[6] under fix_scale); computeScale
// reads what it leaves.
template <int N, class Est, class Oplus>
__device__ inline void next_trial(State<N, Est>& c, double* L, double* y, Oplus&& oplus) {
    double x[N];
    const bool ok = cholesky_solve<N>(c.H, c.b, c.lambda, x, L, y);
    if (ok) {
        const Est est = c.est;
        Est trial;
        oplus(est, x, trial);
        c.trial = trial;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = 0.0;
        c.trial = c.est;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) c.x[i] = x[i];
    c.ok = ok ? 1 : 0;
    c.phase = kTrial;
}

template <int N, class Est, class Oplus>
__device__ inline void begin_iteration(State<N, Est>& c, double* L, double* y, Oplus&& oplus) {
    c.iter += 1;
    c.ini_chi = c.chi;
    c.qmax = 0;
    next_trial(c, L, y, oplus);
}

// OptimizationAlgorithmLevenberg::solve, one pass at a time: c.tot holds the sums of the pass
// c.phase asked for.  TrialBuilds: a trial pass delivers the whole system at c.trial, so an
// accepted trial's (H, b) is the next iteration's and that iteration begins at once; otherwise a
// trial pass delivers the robust chi2 alone and a build pass at c.est follows (kRebuild).
template <bool TrialBuilds, int N, class Est, class Oplus>
__device__ inline void step(State<N, Est>& c, double* L, double* y, Oplus&& oplus) {
    constexpr int U = State<N, Est>::kUpper;
    auto take_system = [&c] {
        for (int i = 0; i < U; ++i) c.H[i] = c.tot[i];
        for (int i = 0; i < N; ++i) c.b[i] = c.tot[U + i];
    };
    if (c.phase != kTrial) {  // a build pass at c.est: the iteration's system and chi2
        take_system();
        c.chi = c.tot[U + N];
        if (c.phase == kInit) {
            double max_diag = 0.0;
            for (int j = 0; j < N; ++j) {  // std::max(fabs(h), maxDiagonal)
                const double a = fabs(c.H[upper_index<N>(j, j)]);
                max_diag = a < max_diag ? max_diag : a;
            }
            c.lambda = kTau * max_diag;
            c.ni = 2.0;
            c.stop_bad = 0;
        }
        begin_iteration(c, L, y, oplus);
        return;
    }
    const double tmp_chi = c.ok ? c.tot[U + N] : DBL_MAX;
    double scale = 0.0;
    for (int j = 0; j < N; ++j) scale += c.x[j] * (c.lambda * c.x[j] + c.b[j]);
    scale += kScaleGuard;
    const double rho = (c.chi - tmp_chi) / scale;
    if (rho > 0 && isfinite(tmp_chi)) {
        const double t3 = 2.0 * rho - 1.0;
        double alpha = 1.0 - (t3 * t3) * t3;
        alpha = alpha < kAlphaMax ? alpha : kAlphaMax;
        c.lambda *= (kAlphaMin < alpha ? alpha : kAlphaMin);
        c.ni = 2.0;
        c.chi = tmp_chi;
        c.est = c.trial;
        if (TrialBuilds) take_system();
    } else {
        c.lambda *= c.ni;
        c.ni *= 2.0;
        c.rejected += 1;
    }
    c.qmax += 1;
    if (rho < 0 && c.qmax < kMaxTrials) {
        next_trial(c, L, y, oplus);
        return;
    }
    if (c.qmax == kMaxTrials || rho == 0) {
        c.done = 1;
        return;
    }
    if ((c.ini_chi - c.chi) * kStopGain < c.ini_chi)
        c.stop_bad += 1;
    else
        c.stop_bad = 0;
    if (c.stop_bad >= kMaxBadIterations || c.iter >= c.max_iter) {
        c.done = 1;
        return;
    }
    if (TrialBuilds)
        begin_iteration(c, L, y, oplus);
    else
        c.phase = kRebuild;  // the next iteration's computeActiveErrors + buildSystem at c.est
}

// ------------------------------------------------------------------ Huber, quaternions, Rodrigues

// RobustKernelHuber::robustify
__device__ __forceinline__ void huber(double chi2, double delta, double dsqr, double& rho0, double& rho1) {
    rho0 = chi2, rho1 = 1.0;
    if (!(chi2 <= dsqr)) {
        const double sq = __dsqrt_rn(chi2);
        rho0 = (2.0 * sq) * delta - dsqr;
        rho1 = delta / sq;
    }
}

template <int I>
__device__ __forceinline__ void quat_from_R_branch(const double (&R)[9], double (&q)[4]) {
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = __dsqrt_rn(((R[4 * I] - R[4 * J]) - R[4 * K]) + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3 * K + J] - R[3 * J + K]) * t;
    q[J] = (R[3 * J + I] + R[3 * I + J]) * t;
    q[K] = (R[3 * K + I] + R[3 * I + K]) * t;
}

// Eigen: Quaterniond(Matrix3d), R row-major; not normalised
__device__ inline void quat_from_R(const double (&R)[9], double (&q)[4]) {
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
        if (R[8] > (i == 1 ? R[4] : R[0])) i = 2;
        if (i == 0)
            quat_from_R_branch<0>(R, q);
        else if (i == 1)
            quat_from_R_branch<1>(R, q);
        else
            quat_from_R_branch<2>(R, q);
    }
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

// Eigen's quaternion product a * b (Hamilton); not normalised.  out may be neither a nor b.
__device__ __forceinline__ void quat_mul(const double (&a)[4], const double (&b)[4], double (&out)[4]) {
    out[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    out[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    out[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    out[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}

constexpr double kSmallAngle = 0.00001;  // se3quat.h:232, sim3.h:84

// the rotation part of SE3Quat::exp and Sim3(Vector7d): O = [omega]x, O2 = O O,
// R = I + sin(theta) / theta O + (1 - cos(theta)) / theta^2 O2, and I + O + O2 below kSmallAngle;
// returns theta = |omega|
__device__ inline double rodrigues(double om0, double om1, double om2, double (&O)[3][3], double (&O2)[3][3],
                                   double (&R)[9]) {
    const double theta = __dsqrt_rn((om0 * om0 + om1 * om1) + om2 * om2);
    const double Ox[3][3] = {{0.0, -om2, om1}, {om2, 0.0, -om0}, {-om1, om0, 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            O[i][j] = Ox[i][j];
            O2[i][j] = (Ox[i][0] * Ox[0][j] + Ox[i][1] * Ox[1][j]) + Ox[i][2] * Ox[2][j];
        }
    if (theta < kSmallAngle) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double a = sin(theta) / theta;
        const double b = (1.0 - cos(theta)) / (theta * theta);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
    }
    return theta;
}

// ------------------------------------------------------------------ the workgroup sum (every lane)

// Fixed-order sum of acc[first..last] over the workgroup of T lanes: 16-lane rows on DPP, one LDS
// row per 16 lanes, then lane v of first..last adds the rows of value v in order and returns its
// total (0 in every other lane).  No floating-point atomics: the bits do not depend on the block's
// neighbours or on the call.  One barrier inside; s_part is free again after the caller's next.
template <int T, int kVals>
__device__ __forceinline__ double block_sum(double (&acc)[kVals], double (&s_part)[T / 16][kVals], int first,
                                            int last) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int v = 0; v < kVals; ++v)
        if (first <= v && v <= last) acc[v] = row16_sum(acc[v]);
    if ((tid & 15) == 0) {
#pragma unroll
        for (int v = 0; v < kVals; ++v)
            if (first <= v && v <= last) s_part[tid >> 4][v] = acc[v];
    }
    __syncthreads();
    double sum = 0.0;
    if (first <= tid && tid <= last) {
        sum = s_part[0][tid];
        for (int r = 1; r < T / 16; ++r) sum += s_part[r][tid];
    }
    return sum;
}

}  // namespace lm
}  // namespace orbgpu
