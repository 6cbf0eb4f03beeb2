// sim3opt.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cpp:1229-1433) for a
// batch of loop candidates (include/orbgpu_sim3opt.h): the refinement of one
// Sim3 against its correspondences by reprojection in both keyframes, with
// g2o's Levenberg-Marquardt (core/optimization_algorithm_levenberg.cpp:61-189),
// the binary edges' numeric Jacobians and robust quadratic form
// (core/base_binary_edge.hpp:131-204, 91-113), Huber
// (core/robust_kernel_impl.cpp:64-91), the two Sim3 projection edges
// (types/types_seven_dof_expmap.h:61-90, 131-172) and Sim3 (types/sim3.h).
// tests/sim3opt_ref.py is the same arithmetic, expression for expression.
// The LM state machine, the 7x7 solve, Huber, the quaternion algebra, the
// workgroup sum and the matrix write-out are lm_device.h's, shared with
// poseopt.hip; this file adds the Sim3 update (sim3opt_device.h), the two
// edges with their numeric Jacobians and the two optimisations with their checks.
//
// One workgroup per job, one launch for both optimisations and both checks.
// Correspondence i of a job belongs to lane i % T for the whole call: the lane
// reads it (from LDS when the job has at most kCap correspondences, else from
// HBM/L2), keeps its flag and adds its two edges' terms to 36 private doubles
// -- the 28 upper entries of H, the 7 of b and the robust chi2.  The sums are
// reduced in a fixed order (lm::block_sum): a job's bits do not depend on its
// neighbours, its block index or the call.
//
// Two kinds of pass.  A *build* pass is g2o's computeActiveErrors +
// buildSystem at the estimate: lanes 0..14 first leave the estimate, its 14
// perturbed copies oplus(+-1e-9 e_d) and all 15 inverses in LDS (they do not
// depend on the edge), then every lane evaluates its edges at the 15 states
// (30 projections per correspondence) and accumulates the 36 sums.  A *trial*
// pass evaluates the edges at the trial estimate alone and reduces one sum,
// the robust chi2.  The system is therefore built once per LM iteration, as in
// g2o, and a rejected trial costs 2 projections per correspondence instead of
// 30; the price is one extra pass (four barriers) per accepted iteration.  At
// convergence most trials are rejected (up to ten per iteration), so this is
// the cheaper choice; the bits are the same either way.
//
// After each pass lane 0 advances the LM state machine in LDS (lm::step: accept /
// reject, lambda, the stop rules, the next solve and Sim3(x) * estimate) and
// leaves `phase` and `done` there; every lane reads those words after the
// barrier, so no lane ever decides from a sum of its own.  The loop bound,
// 10 x (1 + 10) passes, is the reference's 10 iterations of 10 trials; the
// kernel ends on any input.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/orbgpu_sim3opt.h"
#include "host_common.h"
#include "host_ctx.h"
#include "sim3opt_device.h"

namespace {

namespace lm = orbgpu::lm;
using orbgpu::sim3opt::Sim3;
using Lm = lm::State<7, Sim3>;

constexpr int kCap = 768;    // correspondences of a job kept in LDS (12 floats and a flag byte each)
constexpr int kVals = Lm::kVals;  // H (28), b (7), robust chi2
constexpr int kStates = 15;  // the estimate and oplus(+-1e-9 e_d), d = 0..6
constexpr int kMaxPasses = 110;
constexpr int kThreads = 256;
constexpr double kDelta = 1e-9;                  // base_binary_edge.hpp:147
constexpr double kScalar = 1.0 / (2 * kDelta);   // :148

// the job's state in LDS; written by lane 0 between barriers, read by all
struct Ctl {
    Lm lm;
    double L[28], y[7];       // the solve's Cholesky factor and forward substitution
    double delta, dsqr, th2;  // Huber's (float)sqrt(th2), its float square; th2
    double K1[4], K2[4];
    int n, offset, valid, fix_scale, n_bad;
    int lm_iterations[2], lm_rejected[2];
};

// VertexSim3Expmap::oplusImpl of u on est
__device__ inline void oplus(const Sim3& est, double (&u)[7], bool fix_scale, Sim3& out) {
    if (fix_scale) u[6] = 0.0;
    Sim3 e;
    orbgpu::sim3opt::sim3_exp(u, e);
    orbgpu::sim3opt::sim3_mul(e, est, out);
}

// ------------------------------------------------------------------ the edges (every lane)

// what one edge of a correspondence reads: the fixed vertex' point, the keypoint, the information
struct EdgeIn {
    double P[3], o[2], w;
};

// obs - cam_map(project(S.map(P))), S in LDS
__device__ __forceinline__ void project_error(const Sim3& S, const double (&P)[3], const double (&o)[2],
                                              const double* K, double& e0, double& e1) {
    const double q[4] = {S.q[0], S.q[1], S.q[2], S.q[3]};
    double r0, r1, r2;
    lm::quat_rotate(q, P[0], P[1], P[2], r0, r1, r2);
    const double s = S.s;
    const double x = s * r0 + S.t[0];
    const double y = s * r1 + S.t[1];
    const double z = s * r2 + S.t[2];
    e0 = o[0] - ((x / z) * K[0] + K[2]);
    e1 = o[1] - ((y / z) * K[1] + K[3]);
}

// one edge's linearizeOplus + constructQuadraticForm: `states` are the 15 estimates the edge maps
// its point with (S for e12, S^-1 for e21)
__device__ __forceinline__ void add_edge(double (&acc)[kVals], const Sim3* states, const double (&P)[3],
                                         const double (&o)[2], const double* K, double w, double delta,
                                         double dsqr) {
    double e[2];
    project_error(states[0], P, o, K, e[0], e[1]);
    const double chi2 = e[0] * (w * e[0]) + e[1] * (w * e[1]);
    double rho0, rho1;
    lm::huber(chi2, delta, dsqr, rho0, rho1);
    double J[7][2];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        // the states do not depend on the edge: without this the compiler reads all 30 of them from
        // LDS ahead of the loop over the lane's correspondences and spills them
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        double p0, p1, m0, m1;
        project_error(states[1 + 2 * d], P, o, K, p0, p1);
        __builtin_amdgcn_sched_barrier(0);
        project_error(states[2 + 2 * d], P, o, K, m0, m1);
        J[d][0] = kScalar * (p0 - m0);
        J[d][1] = kScalar * (p1 - m1);
    }
    const double W = rho1 * w;  // robustInformation
    const double omr[2] = {(-(w * e[0])) * rho1, (-(w * e[1])) * rho1};
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        __builtin_amdgcn_sched_barrier(0);  // one row of H at a time: the 28 products are independent
        const double wj0 = W * J[j][0], wj1 = W * J[j][1];
#pragma unroll
        for (int k = j; k < 7; ++k) acc[lm::upper_index<7>(j, k)] += wj0 * J[k][0] + wj1 * J[k][1];
        acc[28 + j] += J[j][0] * omr[0] + J[j][1] * omr[1];
    }
    acc[35] += rho0;
}

// the batch arrays and where the job's correspondences are
struct Src {
    const float *P1c, *P2c, *obs1, *obs2, *w1, *w2;
    size_t base;
    bool on_chip;
};

// edge 0 is e12 (P2c mapped by S into keyframe 1), edge 1 is e21 (P1c mapped by S^-1 into keyframe 2)
__device__ __forceinline__ EdgeIn load_edge(const float (&s_corr)[12][kCap], const Src& src, int i, int edge) {
    EdgeIn e;
    if (src.on_chip) {
#pragma unroll
        for (int k = 0; k < 3; ++k) e.P[k] = (double)s_corr[(edge ? 0 : 3) + k][i];
#pragma unroll
        for (int k = 0; k < 2; ++k) e.o[k] = (double)s_corr[(edge ? 8 : 6) + k][i];
        e.w = (double)s_corr[edge ? 11 : 10][i];
    } else {
        const float* P = edge ? src.P1c : src.P2c;
        const float* o = edge ? src.obs2 : src.obs1;
        const float* w = edge ? src.w2 : src.w1;
        // the addresses are formed here, from an index the compiler cannot follow: otherwise it keeps
        // six running pointers per lane alive through the whole kernel (registers the on-chip path needs)
        asm volatile("" : "+v"(i));
        const size_t at = src.base + (size_t)i;
#pragma unroll
        for (int k = 0; k < 3; ++k) e.P[k] = (double)P[3 * at + k];
#pragma unroll
        for (int k = 0; k < 2; ++k) e.o[k] = (double)o[2 * at + k];
        e.w = (double)w[at];
    }
    return e;
}

// computeError + chi2() of one edge at `S` (the estimate for e12, its inverse for e21)
__device__ __forceinline__ double edge_chi2(const EdgeIn& e, const Sim3& S, const double* K) {
    double e0, e1;
    project_error(S, e.P, e.o, K, e0, e1);
    return e0 * (e.w * e0) + e1 * (e.w * e1);
}

// Register budget of two waves per SIMD (256 VGPRs), i.e. two workgroups per CU: left to itself the
// compiler takes 494 and fits one.  The build's sim3opt.s must show no private segment.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void sim3opt_kernel(
    const orbgpu_sim3opt_job* __restrict__ jobs, int total_corr, const float* __restrict__ P1c,
    const float* __restrict__ P2c, const float* __restrict__ obs1, const float* __restrict__ obs2,
    const float* __restrict__ w1, const float* __restrict__ w2, orbgpu_sim3opt_result* __restrict__ results,
    uint8_t* __restrict__ removed) {
    constexpr int T = kThreads;
    __shared__ Ctl ctl;
    __shared__ double s_part[T / 16][kVals];
    __shared__ Sim3 s_S[kStates], s_Sinv[kStates];
    __shared__ float s_corr[12][kCap];
    __shared__ uint8_t s_flag[kCap];

    const int tid = threadIdx.x;
    const orbgpu_sim3opt_job* job = jobs + blockIdx.x;
    if (tid == 0) {
        const int n = job->n, offset = job->offset;
        const bool valid = n >= 0 && offset >= 0 && (long long)offset + n <= (long long)total_corr;
        ctl.valid = valid ? 1 : 0;
        ctl.n = valid ? n : 0;
        ctl.offset = valid ? offset : 0;
        ctl.fix_scale = job->fix_scale;
        for (int k = 0; k < 4; ++k) {
            ctl.lm.est.q[k] = job->q12[k];
            ctl.K1[k] = (double)job->K1[k];
            ctl.K2[k] = (double)job->K2[k];
        }
        for (int k = 0; k < 3; ++k) ctl.lm.est.t[k] = job->t12[k];
        ctl.lm.est.s = job->s12;
        ctl.lm.trial = ctl.lm.est;
        const float th2 = job->th2;
        const float delta = (float)__dsqrt_rn((double)th2);  // const float deltaHuber = sqrt(th2)
        ctl.th2 = (double)th2;
        ctl.delta = (double)delta;
        ctl.dsqr = (double)(float)((double)delta * (double)delta);  // robust_kernel_impl.h:85: float dsqr
        ctl.n_bad = 0;
        for (int k = 0; k < 2; ++k) ctl.lm_iterations[k] = 0, ctl.lm_rejected[k] = 0;
    }
    __syncthreads();
    // the same for every lane: kept in scalar registers
    const int n = __builtin_amdgcn_readfirstlane(ctl.n);
    const size_t base = (size_t)__builtin_amdgcn_readfirstlane(ctl.offset);
    const bool on_chip = n <= kCap;
    const bool fix_scale = __builtin_amdgcn_readfirstlane(ctl.fix_scale) != 0;
    const double* K1 = ctl.K1;  // the constants of the job are read from LDS where they are used
    const double* K2 = ctl.K2;
    uint8_t* g_flag = removed + base;

    for (int i = tid; i < n; i += T) {
        if (on_chip) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_corr[k][i] = P1c[3 * (base + i) + k];
                s_corr[3 + k][i] = P2c[3 * (base + i) + k];
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                s_corr[6 + k][i] = obs1[2 * (base + i) + k];
                s_corr[8 + k][i] = obs2[2 * (base + i) + k];
            }
            s_corr[10][i] = w1[base + i];
            s_corr[11][i] = w2[base + i];
            s_flag[i] = 0;
        } else {
            g_flag[i] = 0;
        }
    }
    // lane i % T alone touches correspondence i, its LDS copy and its flag: no barrier is needed for them

    const Src src = {P1c, P2c, obs1, obs2, w1, w2, base, on_chip};
    // the LM step's update; fix_scale by value: a reference would give it an address in scratch
    const auto update = [fix_scale](const Sim3& est, double (&u)[7], Sim3& out) { oplus(est, u, fix_scale, out); };

    int rounds = 0, n_bad_first = 0, n_in = 0;               // uniform: read from ctl after barriers
    for (int round = 0; round < 2 && n > 0; ++round) {
        if (tid == 0) {
            // initializeOptimization + optimize(): lambda, ni and the stop counter start afresh at
            // iteration 0, the estimate is the vertex' (the first optimisation's result in round 1)
            lm::start(ctl.lm, round == 0 ? 5 : (n_bad_first > 0 ? 10 : 5));
            ctl.n_bad = 0;
        }
        __syncthreads();

        for (int pass = 0; pass < kMaxPasses; ++pass) {
            const bool build = ctl.lm.phase != lm::kTrial;
            if (tid < (build ? kStates : 1)) {
                Sim3 S;
                if (!build) {
                    S = ctl.lm.trial;
                } else if (tid == 0) {
                    S = ctl.lm.est;
                } else {
                    const int d = (tid - 1) >> 1;
                    const double step = (tid & 1) ? kDelta : -kDelta;
                    double u[7];
#pragma unroll
                    for (int k = 0; k < 7; ++k) u[k] = k == d ? step : 0.0;
                    const Sim3 est = ctl.lm.est;
                    oplus(est, u, fix_scale, S);
                }
                Sim3 Sinv;
                orbgpu::sim3opt::sim3_inverse(S, Sinv);
                s_S[tid] = S;
                s_Sinv[tid] = Sinv;
            }
            __syncthreads();

            double acc[kVals];
#pragma unroll
            for (int v = 0; v < kVals; ++v) acc[v] = 0.0;
            for (int i = tid; i < n; i += T) {
                if (on_chip ? s_flag[i] : g_flag[i]) continue;  // removeEdge
                const double delta = ctl.delta, dsqr = ctl.dsqr;
                if (build) {
                    // e12, then e21: a rolled loop, so that the two edges' 15 evaluations are not
                    // interleaved (twice the registers)
#pragma unroll 1
                    for (int edge = 0; edge < 2; ++edge) {
                        const EdgeIn e = load_edge(s_corr, src, i, edge);
                        add_edge(acc, edge ? s_Sinv : s_S, e.P, e.o, edge ? K2 : K1, e.w, delta, dsqr);
                    }
                } else {
#pragma unroll 1
                    for (int edge = 0; edge < 2; ++edge) {
                        double rho0, rho1;
                        const EdgeIn e = load_edge(s_corr, src, i, edge);
                        lm::huber(edge_chi2(e, edge ? s_Sinv[0] : s_S[0], edge ? K2 : K1), delta, dsqr, rho0, rho1);
                        acc[35] += rho0;
                    }
                }
            }
            const double sum = lm::block_sum<T>(acc, s_part, build ? 0 : kVals - 1, kVals - 1);
            if (tid < kVals && (build || tid == kVals - 1)) ctl.lm.tot[tid] = sum;
            __syncthreads();
            if (tid == 0) lm::step<false>(ctl.lm, ctl.L, ctl.y, update);
            __syncthreads();
            if (ctl.lm.done) break;
        }

        // the check (Optimizer.cpp:1377-1394, :1411-1425): chi2() of an edge still in the graph is
        // the error of the last trial evaluated, accepted or not; s_S[0] / s_Sinv[0] still hold it
        {
            int bad = 0;
            const double th2 = ctl.th2;
            for (int i = tid; i < n; i += T) {
                if (on_chip ? s_flag[i] : g_flag[i]) continue;
                const double chi12 = edge_chi2(load_edge(s_corr, src, i, 0), s_S[0], K1);
                const double chi21 = edge_chi2(load_edge(s_corr, src, i, 1), s_Sinv[0], K2);
                if (chi12 > th2 || chi21 > th2) {
                    if (on_chip)
                        s_flag[i] = 1;
                    else
                        g_flag[i] = 1;
                    bad += 1;
                }
            }
            if (bad) atomicAdd(&ctl.n_bad, bad);  // integers: any order gives the same sum
        }
        __syncthreads();
        if (tid == 0) {
            ctl.lm_iterations[round] = ctl.lm.iter;
            ctl.lm_rejected[round] = ctl.lm.rejected;
        }
        const int n_bad = __builtin_amdgcn_readfirstlane(ctl.n_bad);
        rounds = round + 1;
        if (round == 0) {
            n_bad_first = n_bad;
            if (n - n_bad < 10) break;  // return 0: g2oS12 is not written
        } else {
            n_in = (n - n_bad_first) - n_bad;
        }
        __syncthreads();  // lane 0 resets ctl.n_bad next
    }
    __syncthreads();

    if (on_chip && ctl.valid) {
        for (int i = tid; i < n; i += T) g_flag[i] = s_flag[i];
    }
    if (tid == 0) {
        orbgpu_sim3opt_result* r = results + blockIdx.x;
        r->n_in = ctl.valid ? n_in : -1;
        r->rounds = ctl.valid ? rounds : -1;
        r->n_bad_first = n_bad_first;
        for (int k = 0; k < 2; ++k) r->lm_iterations[k] = ctl.lm_iterations[k], r->lm_rejected[k] = ctl.lm_rejected[k];
        r->pad = 0;
        if (rounds == 2) {
            for (int k = 0; k < 4; ++k) r->q12[k] = ctl.lm.est.q[k];
            for (int k = 0; k < 3; ++k) r->t12[k] = ctl.lm.est.t[k];
            r->s12 = ctl.lm.est.s;
        } else {
            for (int k = 0; k < 4; ++k) r->q12[k] = job->q12[k];
            for (int k = 0; k < 3; ++k) r->t12[k] = job->t12[k];
            r->s12 = job->s12;
        }
        lm::write_T16(r->q12, r->t12, r->s12, r->T12);  // Converter::toCvMat(g2o::Sim3)
    }
}

// the result of a job that runs nothing (n == 0), written by the host
void empty_result(const orbgpu_sim3opt_job& j, orbgpu_sim3opt_result& r) {
    std::memset(&r, 0, sizeof(r));
    std::memcpy(r.q12, j.q12, sizeof(j.q12));
    std::memcpy(r.t12, j.t12, sizeof(j.t12));
    std::memcpy(&r.s12, &j.s12, sizeof(j.s12));
    lm::write_T16(j.q12, j.t12, j.s12, r.T12);
}

}  // namespace

extern "C" int orbgpu_optimize_sim3_batch_device(int batch, const orbgpu_sim3opt_job* d_jobs, int total_corr,
                                                 const float* d_P1c, const float* d_P2c, const float* d_obs1,
                                                 const float* d_obs2, const float* d_inv_sigma2_1,
                                                 const float* d_inv_sigma2_2, orbgpu_sim3opt_result* d_results,
                                                 uint8_t* d_removed, void* stream) {
    if (int rc = orbgpu::check_batch_args(
            batch, total_corr, "total_corr", d_jobs && d_results,
            d_P1c && d_P2c && d_obs1 && d_obs2 && d_inv_sigma2_1 && d_inv_sigma2_2 && d_removed, "correspondence"))
        return rc;
    if (batch == 0) return ORBGPU_OK;
    if (int rc = orbgpu::check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sim3opt_kernel, dim3(batch), dim3(kThreads), 0, s, d_jobs, total_corr, d_P1c, d_P2c, d_obs1,
                       d_obs2, d_inv_sigma2_1, d_inv_sigma2_2, d_results, d_removed);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_optimize_sim3_batch(int batch, const orbgpu_sim3opt_job* jobs, int total_corr,
                                          const float* P1c, const float* P2c, const float* obs1, const float* obs2,
                                          const float* inv_sigma2_1, const float* inv_sigma2_2,
                                          orbgpu_sim3opt_result* results, uint8_t* removed) {
    using namespace orbgpu;
    int rc = check_batch_args(batch, total_corr, "total_corr", jobs && results,
                              P1c && P2c && obs1 && obs2 && inv_sigma2_1 && inv_sigma2_2 && removed, "correspondence");
    if (rc || (rc = check_job_ranges(batch, jobs, total_corr))) return rc;
    if (batch == 0) return ORBGPU_OK;
    if (total_corr == 0) {  // every job has n == 0: nothing to optimise, nothing to launch
        for (int b = 0; b < batch; ++b) empty_result(jobs[b], results[b]);
        return ORBGPU_OK;
    }
    if ((rc = check_device())) return rc;
    const size_t tc = (size_t)total_corr;
    HostCtx* ctx;
    if ((rc = host_ctx(&ctx))) return rc;
    HostCall call(*ctx);
    const orbgpu_sim3opt_job* dj;
    const float *dp1, *dp2, *do1, *do2, *dw1, *dw2;
    orbgpu_sim3opt_result* dr;
    uint8_t* dflag;
    rc = call.run([&](HostCall& A) {
        dj = A.in(jobs, (size_t)batch);
        dp1 = A.in(P1c, 3 * tc);
        dp2 = A.in(P2c, 3 * tc);
        do1 = A.in(obs1, 2 * tc);
        do2 = A.in(obs2, 2 * tc);
        dw1 = A.in(inv_sigma2_1, tc);
        dw2 = A.in(inv_sigma2_2, tc);
        dflag = A.inout(removed, tc);  // bytes outside every job's range keep the caller's values
        dr = A.out<orbgpu_sim3opt_result>((size_t)batch);
    });
    if (rc) return rc;
    rc = orbgpu_optimize_sim3_batch_device(batch, dj, total_corr, dp1, dp2, do1, do2, dw1, dw2, dr, dflag,
                                           ctx->stream);
    if (rc) return rc;
    call.fetch(dr, results, sizeof(*dr) * batch);
    call.fetch(dflag, removed, tc);
    return call.finish();
}
