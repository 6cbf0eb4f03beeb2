// poseopt.hip -- Optimizer::PoseOptimization (src/Optimizer.cpp:291-513) for a
// batch of frames (include/orbgpu_poseopt.h): the motion-only refinement of one
// 6-DoF pose against its MapPoint observations, with g2o's Levenberg-Marquardt
// (core/optimization_algorithm_levenberg.cpp:61-189), the unary edges'
// quadratic form (core/base_unary_edge.hpp:43-72), Huber
// (core/robust_kernel_impl.cpp:64-91), the two OnlyPose edges
// (types/types_six_dof_expmap.cpp:285-385) and SE3Quat (types/se3quat.h).
// tests/poseopt_ref.py is the same arithmetic, expression for expression.
// The LM state machine, the 6x6 solve, Huber, the quaternion algebra, the
// workgroup sum and the matrix write-out are lm_device.h's, shared with
// sim3opt.hip; the Huber thresholds are projection_edge.h's.  This file adds
// SE3Quat's exp(x) * estimate, the two OnlyPose edges and the four rounds with
// their classification.  Its SE3Quat and computeError are the text of
// se3_device.h and projection_edge.h: calling those instead compiled this
// kernel to other code, which measured up to 2 % slower at 300 edges a job for
// a reason that was not found, so the kernel keeps its own.
//
// One workgroup per job, one launch for the whole optimisation.  Edge i of a
// job belongs to lane i % T for the whole call: the lane reads it (from LDS
// when the job has at most kCap edges, else from HBM/L2), keeps its flag and
// adds its terms to 28 private doubles -- the 21 upper entries of H, b and the
// robust chi2.  One "pass" evaluates every active edge at the trial estimate
// and reduces the 28 sums in a fixed order (lm::block_sum): a job's bits do
// not depend on its neighbours, its block index or the call.
//
// The passes of a round are one flat loop.  After each pass lane 0 advances the
// LM state machine in LDS (lm::step: accept / reject, lambda, the stop rules,
// the next solve and exp(x) * estimate) and leaves `done` there; every lane reads
// that word after the barrier, so no lane ever decides from a sum of its own.
// The system (H, b) is built in the same pass that gives a trial its chi2: an
// accepted trial's system is the next iteration's, a rejected trial keeps the
// old one, and neither is recomputed (the values would be the same bits).  The
// loop bound, 1 + 10 x 10 passes, is the reference's 10 iterations of 10
// trials; the kernel ends on any input.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/orbgpu_poseopt.h"
#include "host_common.h"
#include "host_ctx.h"
#include "lm_device.h"
#include "projection_edge.h"

namespace {

namespace lm = orbgpu::lm;

constexpr int kCap = 1536;  // edges of a job kept in LDS (7 floats and a flag byte each)
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
using Lm = lm::State<6, Se3>;
constexpr int kVals = Lm::kVals;  // H (21), b (6), robust chi2
constexpr int kIterations = 10;   // optimizer.optimize(its[it]), Optimizer.cpp:441
constexpr int kMaxPasses = 1 + kIterations * lm::kMaxTrials;

using orbgpu::proj_edge::HuberConst;

// the job's state in LDS; written by lane 0 between barriers, read by all
struct Ctl {
    Lm lm;
    Se3 est0;
    int n, offset, valid, rounds, n_bad;
    float fx, fy, cx, cy, bf;
};

// ------------------------------------------------------------------ SE3Quat (lane 0)

// SE3Quat::normalizeRotation
__device__ inline void quat_normalize(double (&q)[4]) {
    if (q[3] < 0) {
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    }
    const double n = __dsqrt_rn(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}

// SE3Quat::exp(x) * est  (se3quat.h:223-257, 104-110)
__device__ void se3_exp_times(const Se3& est, const double (&x)[6], Se3& out) {
    double O[3][3], O2[3][3], R[9], V[3][3];
    const double theta = lm::rodrigues(x[0], x[1], x[2], O, O2, R);
    if (theta < lm::kSmallAngle) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) V[i][j] = R[3 * i + j];
    } else {
        const double sn = sin(theta), cs = cos(theta);
        const double b = (1.0 - cs) / (theta * theta);
        const double d = (theta - sn) / ((theta * theta) * theta);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) V[i][j] = ((i == j ? 1.0 : 0.0) + b * O[i][j]) + d * O2[i][j];
    }
    double te[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) te[i] = (V[i][0] * x[3] + V[i][1] * x[4]) + V[i][2] * x[5];
    double a[4];
    lm::quat_from_R(R, a);
    quat_normalize(a);
    // SE3Quat::operator*: t = ta + qa * tb, q = qa * qb, normalised
    double r0, r1, r2;
    lm::quat_rotate(a, est.t[0], est.t[1], est.t[2], r0, r1, r2);
    double q[4];
    lm::quat_mul(a, est.q, q);
    quat_normalize(q);
    for (int i = 0; i < 4; ++i) out.q[i] = q[i];
    out.t[0] = te[0] + r0;
    out.t[1] = te[1] + r1;
    out.t[2] = te[2] + r2;
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
    lm::quat_rotate(s.q, (double)ed.X[0], (double)ed.X[1], (double)ed.X[2], r0, r1, r2);
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
            if (have) acc[lm::upper_index<6>(j, k)] += c;
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
        double R[9], q[4];
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 3; ++col) R[3 * r + col] = (double)job->Tcw0[4 * r + col];
        lm::quat_from_R(R, q);  // Converter::toSE3Quat
        quat_normalize(q);
        for (int i = 0; i < 4; ++i) ctl.est0.q[i] = q[i];
        for (int r = 0; r < 3; ++r) ctl.est0.t[r] = (double)job->Tcw0[4 * r + 3];
        ctl.lm.est = ctl.est0;
        ctl.lm.trial = ctl.est0;
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
            ctl.lm.est = ctl.est0;  // setEstimate(toSE3Quat(pFrame->mTcw)), every round
            lm::start(ctl.lm, kIterations);
            ctl.n_bad = 0;
        }
        __syncthreads();
        const bool robust = round < 3;  // the kernels are removed after round 2's classification

        for (int pass = 0; pass < kMaxPasses; ++pass) {
            const Se3 s = ctl.lm.trial;
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
                if (robust)
                    lm::huber(chi2, stereo ? hc.delta_stereo : hc.delta_mono,
                              stereo ? hc.dsqr_stereo : hc.dsqr_mono, rho0, rho1);
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
            const double sum = lm::block_sum<T>(acc, s_part, 0, kVals - 1);
            if (tid < kVals) ctl.lm.tot[tid] = tid >= 21 && tid < 27 ? -sum : sum;  // b -= rho1 J^T w e
            __syncthreads();
            if (tid == 0) {
                double L[21], y[6];  // lane 0's registers
                lm::step<true>(ctl.lm, L, y, se3_exp_times);
            }
            __syncthreads();
            if (ctl.lm.done) break;
        }

        // classification (Optimizer.cpp:443-500): an active edge keeps the error of the last
        // trial, accepted or not; a flagged edge is recomputed at the (restored) estimate
        {
            const Se3 s_trial = ctl.lm.trial, s_est = ctl.lm.est;
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
            lm_iterations[round] = ctl.lm.iter;
            lm_rejected[round] = ctl.lm.rejected;
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
            T16[12] = 0.0f, T16[13] = 0.0f, T16[14] = 0.0f, T16[15] = 1.0f;
        } else {  // Converter::toCvMat(SE3Quat)
            lm::write_T16(ctl.lm.est.q, ctl.lm.est.t, 1.0, T16);
        }
    }
}

}  // namespace

extern "C" int orbgpu_pose_optimization_batch_device(int batch, const orbgpu_poseopt_job* d_jobs, int total_obs,
                                                     const float* d_Xw, const float* d_obs,
                                                     const float* d_inv_sigma2, orbgpu_poseopt_result* d_results,
                                                     uint8_t* d_outlier, void* stream) {
    if (int rc = orbgpu::check_batch_args(batch, total_obs, "total_obs", d_jobs && d_results,
                                          d_Xw && d_obs && d_inv_sigma2 && d_outlier, "observation"))
        return rc;
    if (batch == 0) return ORBGPU_OK;
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const HuberConst hc = orbgpu::proj_edge::huber_constants(5.991, 7.815);  // Optimizer.cpp:331-332
    hipLaunchKernelGGL(poseopt_kernel<kThreads>, dim3(batch), dim3(kThreads), 0, s, d_jobs, total_obs, d_Xw, d_obs,
                       d_inv_sigma2, d_results, d_outlier, hc);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_pose_optimization_batch(int batch, const orbgpu_poseopt_job* jobs, int total_obs,
                                              const float* Xw, const float* obs, const float* inv_sigma2,
                                              orbgpu_poseopt_result* results, uint8_t* outlier) {
    using namespace orbgpu;
    int rc = check_batch_args(batch, total_obs, "total_obs", jobs && results, Xw && obs && inv_sigma2 && outlier,
                              "observation");
    if (rc || (rc = check_job_ranges(batch, jobs, total_obs))) return rc;
    if (batch == 0) return ORBGPU_OK;
    if (total_obs == 0) {  // every job has n == 0: nothing to optimise, nothing to launch
        for (int b = 0; b < batch; ++b) {
            std::memset(&results[b], 0, sizeof(results[b]));
            std::memcpy(results[b].Tcw, jobs[b].Tcw0, sizeof(jobs[b].Tcw0));
            results[b].Tcw[15] = 1.0f;
        }
        return ORBGPU_OK;
    }
    if ((rc = check_device())) return rc;
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
