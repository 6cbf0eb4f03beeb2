// reloc.hip -- Tracking::Relocalization's candidate loop on the device
// (include/orbgpu_reloc.h): the PnPsolver set-up of every (lost frame,
// candidate keyframe) pair and the `while (nCandidates > 0 && !bMatch)` loop
// (src/Tracking.cpp:1808-1902) with its whole verification.  One *pass* takes
// every unfinished query through one iterate(5) call of its next live candidate
// and, when that call returns a pose, through the verification; a pass is
// thirteen stages on the caller's stream, every one of them one workgroup per
// query (the PnP hypothesis kernel: one per four hypotheses):
//
//    1 reloc_schedule_kernel   the round-robin cursor, N < mRansacMinInliers ->
//                              bNoMore, n_hyp = max(mRansacMaxIts - mnIterations, 5)
//                              (the `||` of PnPsolver.cpp:224), the 4 * n_hyp draws
//                              from the query's glibc stream resolved through the
//                              swap-remove, and the orbgpu_pnp_problem
//    2 pnp                     orbgpu_pnp_ransac_batch_device, unchanged; the best
//                              mask of every candidate lives in the state block
//    3 reloc_after_pnp_kernel  the stream after exactly the consumed iterations,
//                              mnIterations / mnBestInliers / mBestTcw, bNoMore, the
//                              returned pose (mRefinedTcw, or mBestTcw at bNoMore),
//                              vbInliers -> mvpMapPoints and sFound, the first gather
//    4 poseopt                 orbgpu_pose_optimization_batch_device, unchanged
//    5 reloc_stage_kernel<1>   nGood < 10 ends; the outlier cull; nGood < 50 -> the
//                              KEYFRAME projection call (th 10, ORBdist 100)
//    6 proj                    orbgpu_search_by_projection_batch_device, unchanged
//    7 reloc_stage_kernel<2>   nadditional + nGood >= 50 -> the second gather
//    8 poseopt
//    9 reloc_stage_kernel<3>   30 < nGood < 50 -> sFound rebuilt, the second call
//                              (th 3, ORBdist 64); no outlier cull here
//   10 proj
//   11 reloc_stage_kernel<4>   nGood + nadditional >= 50 -> the third gather
//   12 poseopt
//   13 reloc_stage_kernel<5>   the third cull, nGood >= 50 -> matched; rows, candidate
//                              states, no live candidate -> no match
//
// A query that is not in a stage hands that stage an empty job (n = 0) or an
// idle call.  Nothing synchronises with the host; all values are written with
// plain stores.
#include "../../include/orbgpu_reloc.h"
#include "host_common.h"
#include "ransac_device.h"

namespace orbgpu {

namespace {

using namespace ransacdev;

constexpr int kThreads = 256;
constexpr int kMaxC = ORBGPU_LOOP_MAX_CANDIDATES;
constexpr int kMaxHyp = ORBGPU_RELOC_MAX_ITERATIONS;  // iterations of one iterate() call <= mRansacMaxIts <= 300
constexpr int kMaxKps = 4096;                          // proj_kernel's keypoint capacity
constexpr int kRows = ORBGPU_RELOC_ROWS;

// SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) (Tracking.cpp:1796)
constexpr double kProbability = 0.99;
constexpr int kMinInliers = 10, kMinSet = 4;
constexpr float kEpsilon = 0.5f, kTh2 = 5.991f;

struct Setup {  // SoA, candidate c at c * stride
    float* P3;  // mvP3Dw, 3 per correspondence
    float* P2;  // mvP2D, 2 per correspondence
    float* err; // mvMaxError
    int* kidx;  // mvKeyPointIndices
    int* n;     // per candidate: N (-1: no solver), mRansacMinInliers, mRansacMaxIts
    int* min_inl;
    int* max_its;
};

__host__ __device__ inline Setup carve_setup(void* base, int n_cand, int stride, size_t* bytes) {
    const size_t C = (size_t)(n_cand > 0 ? n_cand : 1), n = C * (size_t)(stride > 0 ? stride : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    Setup w;
    w.P3 = take<float>(p, 3 * n);
    w.P2 = take<float>(p, 2 * n);
    w.err = take<float>(p, n);
    w.kidx = take<int>(p, n);
    w.n = take<int>(p, C);
    w.min_inl = take<int>(p, C);
    w.max_its = take<int>(p, C);
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return w;
}

enum Phase {  // what a query's verification waits for inside a pass
    kIdle = 0,
    kOpt1 = 1,     // the first PoseOptimization
    kSearch1 = 2,  // the first SearchByProjection
    kOpt2 = 3,
    kSearch2 = 4,
    kOpt3 = 5,
    kDecide = 6    // nothing more to run: nGood stands
};

struct QState {  // a query between stages and passes
    int status;         // ORBGPU_RELOC_*
    int phase;          // Phase
    int round, next_c;  // the schedule cursor: the next iterate() call is candidate next_c's in `round`
    int cur_c;          // the candidate whose iterate() call this pass runs, or -1
    int n_hyp;          // iterations laid out for that call
    int calls, verifications, hypotheses;
    int n_good;
    int pad[2];
    orbgpu_rand_state rng;
    float Tcw[16];      // mCurrentFrame.mTcw
};

struct CState {  // a PnPsolver between passes
    int n, min_inl, max_its, its, best, live;
    float best_Tcw[16];  // mBestTcw
};

struct RState {  // the opaque block, carved
    QState* q;
    CState* c;                  // kMaxC per query
    uint8_t* best_mask;         // mvbBestInliers, candidate c at c * stride (persistent)
    uint8_t* refined_mask;      // mvbRefinedInliers of the last Refine()
    orbgpu_pnp_problem* probs;
    orbgpu_pnp_result* pres;
    int* samples;               // 4 * kMaxHyp per query
    int* mp;                    // mvpMapPoints by frame keypoint: the keyframe slot or -1
    int* found;                 // sFound by keyframe slot
    orbgpu_poseopt_job* jobs;
    orbgpu_poseopt_result* opt;
    float *Xw, *obs, *w;        // the gathered observations, query q at q * stride
    int* gidx;                  // their frame keypoints
    uint8_t* outl;              // PoseOptimization's flags per observation
    orbgpu_proj_call* calls;
    int* flags;                 // the call's point flags by keyframe slot
    float* angle;               // pKF->mvKeysUn[i].angle
    uint8_t* occ;               // the frame's occupancy before the call
    int* pm;                    // the call's row and count
    int* pn;
    void* pnp_ws;
};

inline RState carve_state(void* base, int nq, int n_cand, int stride, size_t* bytes) {
    const size_t Q = (size_t)(nq > 0 ? nq : 1), C = (size_t)(n_cand > 0 ? n_cand : 1), S = (size_t)(stride > 0 ? stride : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    RState v;
    v.q = take<QState>(p, Q);
    v.c = take<CState>(p, Q * kMaxC);
    v.best_mask = take<uint8_t>(p, C * S);
    v.refined_mask = take<uint8_t>(p, C * S);
    v.probs = take<orbgpu_pnp_problem>(p, Q);
    v.pres = take<orbgpu_pnp_result>(p, Q);
    v.samples = take<int>(p, Q * 4 * kMaxHyp);
    v.mp = take<int>(p, Q * S);
    v.found = take<int>(p, Q * S);
    v.jobs = take<orbgpu_poseopt_job>(p, Q);
    v.opt = take<orbgpu_poseopt_result>(p, Q);
    v.Xw = take<float>(p, 3 * Q * S);
    v.obs = take<float>(p, 3 * Q * S);
    v.w = take<float>(p, Q * S);
    v.gidx = take<int>(p, Q * S);
    v.outl = take<uint8_t>(p, Q * S);
    v.calls = take<orbgpu_proj_call>(p, Q);
    v.flags = take<int>(p, Q * S);
    v.angle = take<float>(p, Q * S);
    v.occ = take<uint8_t>(p, Q * S);
    v.pm = take<int>(p, Q * S);
    v.pn = take<int>(p, Q);
    v.pnp_ws = reinterpret_cast<void*>(p);
    p += align256(orbgpu_pnp_workspace_bytes((int)(C * S), (int)(Q * kMaxHyp)));
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return v;
}

// ------------------------------------------------------------------ PnPsolver set-up

// PnPsolver::PnPsolver + SetRansacParameters (PnPsolver.cpp:104-195), one block per candidate
__global__ __launch_bounds__(kThreads) void reloc_setup_kernel(const orbgpu_reloc_candidate* __restrict__ cands,
                                                               const orbgpu_reloc_frame* __restrict__ frames,
                                                               const orbgpu_loop_keyframe* __restrict__ kfs,
                                                               const int* __restrict__ match, int stride,
                                                               const int* __restrict__ nmatches, Setup ws,
                                                               int* __restrict__ n_corr) {
    __shared__ int s_wave[kThreads / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (nmatches[c] < ORBGPU_RELOC_MIN_MATCHES) {  // Tracking.cpp:1787-1791: no solver is built
        if (tid == 0) {
            n_corr[c] = -1;
            ws.n[c] = -1;
            ws.min_inl[c] = 0;
            ws.max_its[c] = 0;
        }
        return;
    }
    const orbgpu_reloc_candidate cd = cands[c];
    const orbgpu_reloc_frame& F = frames[cd.frame];
    const orbgpu_loop_keyframe& K = kfs[cd.kf];
    const int* row = match + (size_t)c * stride;
    const size_t o = (size_t)c * stride;
    const int nf = min(F.target.n, stride);
    int base = 0;
    for (int s = 0; s < nf; s += kThreads) {
        const int j = s + tid;
        int slot = -1;
        if (j < nf) {
            slot = row[j];
            if (slot >= K.n || (slot >= 0 && !K.mp_valid[slot])) slot = -1;  // pMP && !pMP->isBad()
        }
        const bool ok = slot >= 0;
        const size_t i = o + compact_slot(ok, lane, wave, s_wave, base);
        if (ok) {
            const orbgpu_keypoint kp = F.target.kps[j];
            for (int k = 0; k < 3; ++k) ws.P3[3 * i + k] = K.mp_world[3 * (size_t)slot + k];
            ws.P2[2 * i] = kp.x;
            ws.P2[2 * i + 1] = kp.y;
            ws.err[i] = F.level_sigma2[kp.octave & 15] * kTh2;  // mvMaxError (:194)
            ws.kidx[i] = j;
        }
        compact_advance<kThreads>(s_wave, base);
        __syncthreads();
    }
    if (tid == 0) {  // SetRansacParameters (:159-190)
        const int N = base;
        int n_min = (int)((float)N * kEpsilon);
        if (n_min < kMinInliers) n_min = kMinInliers;
        if (n_min < kMinSet) n_min = kMinSet;
        float eps = kEpsilon;
        if (eps < (float)n_min / (float)N) eps = (float)n_min / (float)N;
        const int n_it = n_min == N ? 1 : ransac_iterations(kProbability, eps);
        n_corr[c] = N;
        ws.n[c] = N;
        ws.min_inl[c] = n_min;
        ws.max_its[c] = max(1, min(n_it, ORBGPU_RELOC_MAX_ITERATIONS));
    }
}

// ------------------------------------------------------------------ schedule and draw

// a query's candidates; a range outside the candidate table schedules nothing
__device__ __forceinline__ int query_candidates(const orbgpu_reloc_query& Q, int n_cand_total) {
    const bool ok = Q.first_cand >= 0 && Q.n_cand >= 0 && Q.n_cand <= kMaxC && Q.first_cand <= n_cand_total - Q.n_cand;
    return ok ? Q.n_cand : 0;
}

__device__ __forceinline__ void idle_problem(orbgpu_pnp_problem& P) {
    int* w = reinterpret_cast<int*>(&P);
    for (int k = 0; k < (int)(sizeof(orbgpu_pnp_problem) / 4); ++k) w[k] = 0;
}

__global__ __launch_bounds__(kThreads) void reloc_schedule_kernel(
    const orbgpu_reloc_query* __restrict__ queries, int n_cand_total, const orbgpu_reloc_candidate* __restrict__ cands,
    const orbgpu_reloc_frame* __restrict__ frames, const orbgpu_loop_keyframe* __restrict__ kfs,
    const orbgpu_loop_keyframe_search* __restrict__ kss, int stride, Setup ws, int resume, RState V,
    orbgpu_relocalize_result* __restrict__ results, int* __restrict__ rows) {
    __shared__ int c_n[kMaxC], c_min[kMaxC], c_max[kMaxC], c_its[kMaxC], c_best[kMaxC], c_live[kMaxC];
    __shared__ int32_t s_r[31];
    __shared__ int s_over;
    const int q = blockIdx.x, tid = threadIdx.x;
    QState& S = V.q[q];
    CState* CS = V.c + (size_t)q * kMaxC;
    const orbgpu_reloc_query& Q = queries[q];
    const int nc = query_candidates(Q, n_cand_total);
    const int c0 = nc ? Q.first_cand : 0;
    const int status0 = resume ? S.status : ORBGPU_RELOC_PENDING;  // read before any lane writes S
    if (tid == 0) s_over = 0;
    __syncthreads();
    if (resume && status0 != ORBGPU_RELOC_PENDING) {  // finished: the pass does nothing
        if (tid == 0) {
            S.cur_c = -1;
            S.n_hyp = 0;
            S.phase = kIdle;
            idle_problem(V.probs[q]);
        }
        return;
    }
    if (!resume) {
        int* rw = rows + (size_t)q * kRows * stride;
        for (int i = tid; i < kRows * stride; i += kThreads) rw[i] = 0;  // mvbOutlier starts all false (the Frame ctor)
        for (int i = tid; i < stride; i += kThreads) {
            V.mp[(size_t)q * stride + i] = -1;
            V.found[(size_t)q * stride + i] = 0;
        }
        for (int c = 0; c < nc; ++c)  // mvbBestInliers of a new solver
            for (int i = tid; i < stride; i += kThreads) V.best_mask[(size_t)(c0 + c) * stride + i] = 0;
        if (tid < nc) {
            const orbgpu_reloc_candidate cd = cands[c0 + tid];
            const int lim = min(stride, kMaxKps);
            if (frames[cd.frame].target.n > lim || kfs[cd.kf].n > lim || kss[cd.kf].target.n > lim) atomicOr(&s_over, 1);
        }
    }
    if (tid < nc) {
        if (!resume) {
            const int N = ws.n[c0 + tid];
            c_n[tid] = N;
            c_min[tid] = ws.min_inl[c0 + tid];
            c_max[tid] = ws.max_its[c0 + tid];
            c_its[tid] = 0;
            c_best[tid] = 0;
            c_live[tid] = N >= 0;  // no solver: vbDiscarded from the start
            for (int k = 0; k < 16; ++k) CS[tid].best_Tcw[k] = 0.f;
        } else {
            const CState& C = CS[tid];
            c_n[tid] = C.n;
            c_min[tid] = C.min_inl;
            c_max[tid] = C.max_its;
            c_its[tid] = C.its;
            c_best[tid] = C.best;
            c_live[tid] = C.live;
        }
    }
    if (tid < 31) s_r[tid] = resume ? S.rng.r[tid] : Q.rng.r[tid];
    __syncthreads();
    if (tid == 0) {
        orbgpu_relocalize_result& R = results[q];
        int status = ORBGPU_RELOC_PENDING;
        int round = 0, next_c = 0, calls = 0;
        int rf = Q.rng.f, rb = Q.rng.b;
        if (!resume) {  // every word of the result starts at zero
            int* w = reinterpret_cast<int*>(&R);
            for (int k = 0; k < (int)(sizeof(orbgpu_relocalize_result) / 4); ++k) w[k] = 0;
            R.matched = -1;
            R.round = -1;
            R.last_cand = -1;
            R.nadditional[0] = R.nadditional[1] = -1;
            R.rng_after = Q.rng;
            S.rng = Q.rng;
            S.verifications = 0;
            S.hypotheses = 0;
            S.n_good = 0;
            S.pad[0] = S.pad[1] = 0;
            for (int k = 0; k < 16; ++k) S.Tcw[k] = 0.f;
            if (s_over) status = ORBGPU_RELOC_CAPACITY;  // nothing truncated: the query ends
        } else {
            round = S.round;
            next_c = S.next_c;
            calls = S.calls;
            rf = S.rng.f;
            rb = S.rng.b;
        }
        int cur = -1, n_hyp = 0, live = 0;
        for (int c = 0; c < nc; ++c) live += c_live[c];
        while (status == ORBGPU_RELOC_PENDING) {  // `for (i < nKFs)` inside `while (nCandidates > 0 && !bMatch)`
            if (next_c >= nc) {
                if (!live) {
                    status = ORBGPU_RELOC_NO_MATCH;
                    break;
                }
                next_c = 0;
                ++round;
            }
            const int c = next_c;
            if (!c_live[c]) {
                ++next_c;
                continue;
            }
            ++calls;
            R.round = round;
            if (c_n[c] < c_min[c]) {  // PnPsolver.cpp:213-217: bNoMore, no draws, no pose
                c_live[c] = 0;
                --live;
                ++next_c;
                continue;
            }
            cur = c;
            n_hyp = min(max(c_max[c] - c_its[c], ORBGPU_RELOC_ITERATIONS_PER_CALL), kMaxHyp);  // the `||` of :224
            break;
        }
        orbgpu_pnp_problem& P = V.probs[q];
        idle_problem(P);
        if (cur >= 0) {
            const int N = c_n[cur];
            int* smp = V.samples + (size_t)q * 4 * kMaxHyp;
            for (int h = 0; h < n_hyp; ++h) {
                int32_t gen[4];
                int set[4];
                draw_set<4>(N, s_r, rf, rb, gen, set);
                for (int k = 0; k < 4; ++k) smp[4 * h + k] = set[k];
            }
            const orbgpu_proj_target& T = frames[cands[c0 + cur].frame].target;
            P.n = N;
            P.offset = (c0 + cur) * stride;
            P.min_inliers = c_min[cur];
            P.best_inliers = c_best[cur];
            P.n_hyp = n_hyp;
            P.sample_offset = q * kMaxHyp;
            P.fu = T.fx;
            P.fv = T.fy;
            P.uc = T.cx;
            P.vc = T.cy;
        }
        S.status = status;
        S.phase = kIdle;
        S.round = round;
        S.next_c = next_c;
        S.cur_c = cur;
        S.n_hyp = n_hyp;
        S.calls = calls;
        R.status = status;
        R.calls = calls;
    }
    __syncthreads();
    if (tid < nc) {  // empty calls may have discarded candidates
        CState& C = CS[tid];
        C.n = c_n[tid];
        C.min_inl = c_min[tid];
        C.max_its = c_max[tid];
        C.its = c_its[tid];
        C.best = c_best[tid];
        C.live = c_live[tid];
    }
}

// ------------------------------------------------------------------ the glue between the stages

struct Ctx {  // what every glue kernel reads of its query
    const orbgpu_reloc_frame* F;
    const orbgpu_loop_keyframe* K;
    const orbgpu_loop_keyframe_search* KS;
    int nf;  // the frame's keypoints
    int nk;  // the keyframe's slots
};

__device__ __forceinline__ void empty_job(orbgpu_poseopt_job& J, int offset) {
    int* w = reinterpret_cast<int*>(&J);
    for (int k = 0; k < (int)(sizeof(orbgpu_poseopt_job) / 4); ++k) w[k] = 0;
    J.offset = offset;
}

// PoseOptimization's gather (Optimizer.cpp:317-392): the frame keypoints with a MapPoint, ascending
__device__ __forceinline__ void gather_job(const Ctx& X, int q, int stride, const RState& V, const float* Tcw, int* s_wave) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t o = (size_t)q * stride;
    const int* mp = V.mp + o;
    const orbgpu_proj_target& T = X.F->target;
    int base = 0;
    for (int s = 0; s < X.nf; s += kThreads) {
        const int j = s + tid;
        int slot = -1;
        if (j < X.nf) {
            slot = mp[j];
            if (slot >= X.nk) slot = -1;
        }
        const bool ok = slot >= 0;
        const size_t i = o + compact_slot(ok, lane, wave, s_wave, base);
        if (ok) {
            const orbgpu_keypoint kp = T.kps[j];
            for (int k = 0; k < 3; ++k) V.Xw[3 * i + k] = X.K->mp_world[3 * (size_t)slot + k];
            V.obs[3 * i] = kp.x;
            V.obs[3 * i + 1] = kp.y;
            V.obs[3 * i + 2] = T.u_right ? T.u_right[j] : -1.f;
            V.w[i] = X.F->inv_level_sigma2[kp.octave & 15];
            V.gidx[i] = j;
        }
        compact_advance<kThreads>(s_wave, base);
        __syncthreads();
    }
    if (tid == 0) {
        orbgpu_poseopt_job& J = V.jobs[q];
        empty_job(J, q * stride);
        J.n = base;
        for (int k = 0; k < 12; ++k) J.Tcw0[k] = Tcw[k];
        J.fx = T.fx;
        J.fy = T.fy;
        J.cx = T.cx;
        J.cy = T.cy;
        J.bf = T.bf;
    }
}

// what a PoseOptimization leaves in the frame: mvbOutlier where a MapPoint was present, nGood, mTcw
__device__ __forceinline__ void absorb_poseopt(int q, int stride, const RState& V, int* outrow, int which,
                                      orbgpu_relocalize_result& R) {
    const int tid = threadIdx.x;
    const size_t o = (size_t)q * stride;
    const int n = min(V.jobs[q].n, stride);
    for (int i = tid; i < n; i += kThreads) outrow[V.gidx[o + i]] = V.outl[o + i];
    if (tid == 0) {
        const orbgpu_poseopt_result& O = V.opt[q];
        QState& S = V.q[q];
        S.n_good = O.n_good;
        for (int k = 0; k < 16; ++k) S.Tcw[k] = O.Tcw[k];
        const int* src = reinterpret_cast<const int*>(&O);
        int* dst = reinterpret_cast<int*>(&R.opt[which]);
        for (int k = 0; k < (int)(sizeof(orbgpu_poseopt_result) / 4); ++k) dst[k] = src[k];
    }
    __syncthreads();
}

// SearchByProjection(mCurrentFrame, pKF, sFound, th, ORBdist) with matcher2(0.9, true) (Tracking.cpp:1865, :1879)
__device__ __forceinline__ void search_call(const Ctx& X, int q, int stride, const RState& V, float th, int orb_dist) {
    const int tid = threadIdx.x;
    const size_t o = (size_t)q * stride;
    for (int i = tid; i < stride; i += kThreads) {
        V.flags[o + i] = (i < X.nk && X.K->mp_valid[i] && !V.found[o + i]) ? ORBGPU_PT_VALID : 0;
        V.angle[o + i] = i < X.nk ? X.KS->target.kps[i].angle : 0.f;
        V.occ[o + i] = (i < X.nf && V.mp[o + i] >= 0) ? 1 : 0;
    }
    if (tid == 0) {
        orbgpu_proj_call& k = V.calls[q];
        idle_call(k, ORBGPU_PROJ_KEYFRAME);
        k.check_ori = 1;
        k.th = th;
        k.orb_dist = orb_dist;
        k.target = X.F->target;
        k.target.occupied = V.occ + o;
        for (int i = 0; i < 16; ++i) k.target.Tcw[i] = V.q[q].Tcw[i];
        k.points.n = X.nk;
        k.points.flags = V.flags + o;
        k.points.pos = X.K->mp_world;
        k.points.desc = X.KS->mp_desc;
        k.points.min_dist = X.KS->mp_min_dist;
        k.points.max_dist = X.KS->mp_max_dist;
        k.points.angle = V.angle + o;
    }
}

__device__ __forceinline__ Ctx make_ctx(const orbgpu_reloc_query& Q, int c, const orbgpu_reloc_candidate* cands,
                               const orbgpu_reloc_frame* frames, const orbgpu_loop_keyframe* kfs,
                               const orbgpu_loop_keyframe_search* kss, int stride) {
    const orbgpu_reloc_candidate cd = cands[Q.first_cand + c];
    Ctx X;
    X.F = frames + cd.frame;
    X.K = kfs + cd.kf;
    X.KS = kss + cd.kf;
    X.nf = min(X.F->target.n, stride);
    // the two tables describe the same keyframes; the smaller count bounds every index
    X.nk = min(min(X.K->n, X.KS->target.n), stride);
    return X;
}

__global__ __launch_bounds__(kThreads) void reloc_after_pnp_kernel(
    const orbgpu_reloc_query* __restrict__ queries, const orbgpu_reloc_candidate* __restrict__ cands,
    const orbgpu_reloc_frame* __restrict__ frames, const orbgpu_loop_keyframe* __restrict__ kfs,
    const orbgpu_loop_keyframe_search* __restrict__ kss, const int* __restrict__ match, int stride, Setup ws, RState V,
    orbgpu_relocalize_result* __restrict__ results, int* __restrict__ rows) {
    __shared__ int s_wave[kThreads / 64];
    __shared__ int32_t s_r[31];
    __shared__ int s_kind;  // 0: no pose, 1: mRefinedTcw, 2: mBestTcw
    __shared__ float s_T[16];
    const int q = blockIdx.x, tid = threadIdx.x;
    QState& S = V.q[q];
    const int cur = S.cur_c, status = S.status;
    if (tid < 31) s_r[tid] = S.rng.r[tid];
    __syncthreads();
    if (status != ORBGPU_RELOC_PENDING || cur < 0) {
        if (tid == 0) empty_job(V.jobs[q], q * stride);
        return;
    }
    const orbgpu_reloc_query& Q = queries[q];
    const int gc = Q.first_cand + cur;
    const Ctx X = make_ctx(Q, cur, cands, frames, kfs, kss, stride);
    orbgpu_relocalize_result& R = results[q];
    CState& C = V.c[(size_t)q * kMaxC + cur];
    if (tid == 0) {
        const orbgpu_pnp_result P = V.pres[q];
        const int consumed = min(max(P.consumed, 0), S.n_hyp);
        // the stream after exactly the consumed iterations: replayed from the call's start state
        int rf = S.rng.f, rb = S.rng.b;
        for (int k = 0; k < 4 * consumed; ++k) rand_next_raw(s_r, rf, rb);
        for (int k = 0; k < 31; ++k) S.rng.r[k] = R.rng_after.r[k] = s_r[k];
        S.rng.f = R.rng_after.f = rf;
        S.rng.b = R.rng_after.b = rb;
        C.its += consumed;
        C.best = P.best_inliers;
        if (P.best_hyp >= 0)
            for (int k = 0; k < 16; ++k) C.best_Tcw[k] = P.best_Tcw[k];
        S.hypotheses += consumed;
        R.hypotheses = S.hypotheses;
        R.draws = 4 * S.hypotheses;
        int kind = 0;
        if (P.found) {  // return mRefinedTcw (:269-279): bNoMore stays false, the solver stays alive
            kind = 1;
        } else if (C.its >= C.max_its) {  // :284-298
            C.live = 0;
            if (C.best >= C.min_inl) kind = 2;
        }
        S.next_c = cur + 1;
        s_kind = kind;
        if (kind) {
            const float* T = kind == 1 ? P.refined_Tcw : C.best_Tcw;
            for (int k = 0; k < 16; ++k) s_T[k] = S.Tcw[k] = R.pnp_Tcw[k] = R.Tcw[k] = T[k];  // Tcw.copyTo(mTcw)
            R.last_cand = cur;
            R.n_inliers = kind == 1 ? P.refined_inliers : C.best;
            R.refined = kind == 1;
            R.nadditional[0] = R.nadditional[1] = -1;
            R.n_good = 0;
            int* w = reinterpret_cast<int*>(R.opt);
            for (int k = 0; k < (int)(sizeof(R.opt) / 4); ++k) w[k] = 0;
            S.n_good = 0;
            S.phase = kOpt1;
        }
    }
    __syncthreads();
    const int kind = s_kind;
    if (!kind) {
        if (tid == 0) empty_job(V.jobs[q], q * stride);
        return;
    }
    // vbInliers through mvKeyPointIndices; every mvpMapPoints[j] is rewritten, sFound = the inliers'
    // MapPoints (Tracking.cpp:1836-1849)
    const size_t o = (size_t)q * stride, oc = (size_t)gc * stride;
    const uint8_t* mask = (kind == 1 ? V.refined_mask : V.best_mask) + oc;
    const int* row = match + oc;
    int* vb = rows + (size_t)q * kRows * stride;
    const int N = min(max(C.n, 0), stride);
    for (int i = tid; i < stride; i += kThreads) {
        vb[i] = 0;
        V.found[o + i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < N; i += kThreads)
        if (mask[i]) {
            const int j = ws.kidx[oc + i];
            if (j >= 0 && j < stride) vb[j] = 1;
        }
    __syncthreads();
    for (int j = tid; j < stride; j += kThreads) {
        int slot = -1;
        if (j < X.nf && vb[j]) {
            slot = row[j];
            if (slot >= X.nk) slot = -1;
        }
        V.mp[o + j] = slot;
        if (slot >= 0) V.found[o + slot] = 1;
    }
    __syncthreads();
    gather_job(X, q, stride, V, s_T, s_wave);
}

template <int kStage>
__global__ __launch_bounds__(kThreads) void reloc_stage_kernel(
    const orbgpu_reloc_query* __restrict__ queries, const orbgpu_reloc_candidate* __restrict__ cands,
    const orbgpu_reloc_frame* __restrict__ frames, const orbgpu_loop_keyframe* __restrict__ kfs,
    const orbgpu_loop_keyframe_search* __restrict__ kss, int stride, int n_cand_total, RState V,
    orbgpu_relocalize_result* __restrict__ results, orbgpu_reloc_candidate_state* __restrict__ states,
    int* __restrict__ rows) {
    __shared__ int s_wave[kThreads / 64];
    __shared__ float s_T[16];
    constexpr bool kAfterOpt = kStage == 1 || kStage == 3 || kStage == 5;   // the stage reads a PoseOptimization
    constexpr bool kMakesCall = kStage == 1 || kStage == 3;                 // and may ask for a search
    constexpr int kWaits = kStage;  // kOpt1 .. kOpt3 are 1 .. 5 in stage order
    const int q = blockIdx.x, tid = threadIdx.x;
    QState& S = V.q[q];
    const int phase = S.phase, status = S.status, cur = S.cur_c;
    const orbgpu_reloc_query& Q = queries[q];
    orbgpu_relocalize_result& R = results[q];
    const size_t o = (size_t)q * stride;
    int* rw = rows + (size_t)q * kRows * stride;
    int* outrow = rw + 4 * (size_t)stride;  // mvbOutlier
    int* mp = V.mp + o;
    __syncthreads();
    const bool mine = status == ORBGPU_RELOC_PENDING && cur >= 0 && phase == kWaits;
    int next = phase;
    if (mine) {
        const Ctx X = make_ctx(Q, cur, cands, frames, kfs, kss, stride);
        if constexpr (kAfterOpt) {
            absorb_poseopt(q, stride, V, outrow, (kStage - 1) / 2, R);
            const int n_good = S.n_good;
            if constexpr (kStage == 1) {
                if (n_good < 10) {  // `continue` (:1854): no cull, nothing more
                    next = kDecide;
                } else {
                    for (int j = tid; j < X.nf; j += kThreads)  // :1857-1859; sFound keeps the culled points
                        if (outrow[j]) mp[j] = -1;
                    next = n_good < 50 ? kSearch1 : kDecide;
                }
                __syncthreads();
                for (int j = tid; j < stride; j += kThreads) rw[stride + j] = rw[2 * (size_t)stride + j] = mp[j];
            } else if constexpr (kStage == 3) {
                // the outliers of this optimisation keep their MapPoints (:1869-1879)
                for (int j = tid; j < stride; j += kThreads) rw[2 * (size_t)stride + j] = mp[j];
                if (n_good > 30 && n_good < 50) {  // sFound = every MapPoint the frame holds now (:1875-1878)
                    for (int i = tid; i < stride; i += kThreads) V.found[o + i] = 0;
                    __syncthreads();
                    for (int j = tid; j < X.nf; j += kThreads) {
                        const int slot = mp[j];
                        if (slot >= 0 && slot < stride) V.found[o + slot] = 1;
                    }
                    next = kSearch2;
                } else {
                    next = kDecide;
                }
                __syncthreads();
            } else {
                for (int j = tid; j < X.nf; j += kThreads)  // :1886-1888
                    if (outrow[j]) mp[j] = -1;
                next = kDecide;
                __syncthreads();
            }
            if constexpr (kMakesCall) {
                if (next == kSearch1) search_call(X, q, stride, V, 10.f, 100);
                if (next == kSearch2) search_call(X, q, stride, V, 3.f, 64);
            }
        } else {  // after a search: its matches enter mvpMapPoints; -2 entries were only ever this call's own
            const int nadd = V.pn[q];
            const int n_good = S.n_good;
            if (nadd < 0) {  // over the projection matcher's capacity: the query ends, nothing truncated
                next = kIdle;
                if (tid == 0) {
                    S.status = ORBGPU_RELOC_CAPACITY;
                    R.status = ORBGPU_RELOC_CAPACITY;
                    empty_job(V.jobs[q], q * stride);
                }
            } else {
                for (int j = tid; j < X.nf; j += kThreads) {
                    const int p = V.pm[o + j];
                    if (p >= 0 && p < X.nk) mp[j] = p;
                }
                if (tid == 0) R.nadditional[kStage / 2 - 1] = nadd;
                if (tid < 16) s_T[tid] = S.Tcw[tid];
                __syncthreads();
                if (nadd + n_good >= 50) {  // :1867, :1882
                    gather_job(X, q, stride, V, s_T, s_wave);
                    next = kStage == 2 ? kOpt2 : kOpt3;
                } else {
                    if (tid == 0) empty_job(V.jobs[q], q * stride);
                    next = kDecide;
                }
            }
        }
    } else if constexpr (!kAfterOpt) {
        if (tid == 0) empty_job(V.jobs[q], q * stride);
    }
    if constexpr (kMakesCall) {  // no search asked for: the matcher gets an idle call
        const bool searches = mine && (next == kSearch1 || next == kSearch2);
        if (!searches && tid == 0) idle_call(V.calls[q], ORBGPU_PROJ_KEYFRAME);
    }
    if constexpr (kStage < 5) {
        if (tid == 0) S.phase = next;
        return;
    }
    // ---- the decision (:1895-1899) and what the pass leaves behind
    __syncthreads();
    const bool verified = status == ORBGPU_RELOC_PENDING && cur >= 0 && next == kDecide;
    if (verified)
        for (int j = tid; j < stride; j += kThreads) rw[3 * (size_t)stride + j] = mp[j];
    const int nc = query_candidates(Q, n_cand_total);
    const CState* CS = V.c + (size_t)q * kMaxC;
    if (tid < nc) {
        const CState& C = CS[tid];
        orbgpu_reloc_candidate_state& T = states[Q.first_cand + tid];
        T.n = C.n;
        T.min_inliers = C.min_inl;
        T.max_iterations = C.max_its;
        T.iterations = C.its;
        T.best_inliers = C.best;
        T.discarded = C.live ? 0 : 1;
    }
    if (tid == 0) {
        int st = S.status;
        if (verified) {
            S.verifications += 1;
            R.verifications = S.verifications;
            R.n_good = S.n_good;
            for (int k = 0; k < 16; ++k) R.Tcw[k] = S.Tcw[k];
            if (S.n_good >= 50) {
                st = ORBGPU_RELOC_MATCHED;
                R.matched = cur;
            }
        }
        if (st == ORBGPU_RELOC_PENDING) {  // nCandidates == 0: the loops end
            int live = 0;
            for (int c = 0; c < nc; ++c) live += CS[c].live;
            if (!live) st = ORBGPU_RELOC_NO_MATCH;
        }
        S.status = st;
        R.status = st;
        S.phase = kIdle;
    }
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

size_t orbgpu_reloc_setup_workspace_bytes(int n_cand, int match_stride) {
    size_t bytes = 0;
    carve_setup(nullptr, n_cand, match_stride, &bytes);
    return bytes;
}

int orbgpu_reloc_setup_batch_device(int n_cand, const orbgpu_reloc_candidate* d_cands,
                                    const orbgpu_reloc_frame* d_frames, const orbgpu_loop_keyframe* d_kfs,
                                    const int* d_match, int match_stride, const int* d_nmatches, void* d_workspace,
                                    int* d_n_corr, void* stream) {
    if (n_cand < 0 || match_stride <= 0 ||
        (n_cand > 0 && (!d_cands || !d_frames || !d_kfs || !d_match || !d_nmatches || !d_workspace || !d_n_corr)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if ((long long)n_cand * match_stride > 0x7fffffffLL) return fail(ORBGPU_ERR_ARG, "n_cand * match_stride overflows");
    if (n_cand == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    const Setup ws = carve_setup(d_workspace, n_cand, match_stride, nullptr);
    hipLaunchKernelGGL(reloc_setup_kernel, dim3(n_cand), dim3(kThreads), 0, (hipStream_t)stream, d_cands, d_frames, d_kfs,
                       d_match, match_stride, d_nmatches, ws, d_n_corr);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

size_t orbgpu_relocalize_workspace_bytes(int n_queries, int n_cand, int match_stride) {
    const long long C = n_cand > 0 ? n_cand : 1, S = match_stride > 0 ? match_stride : 1, Q = n_queries > 0 ? n_queries : 1;
    if (C * S > 0x7fffffffLL || Q * kMaxHyp > 0x7fffffffLL) return 0;
    size_t bytes = 0;
    carve_state(nullptr, n_queries, n_cand, match_stride, &bytes);
    return bytes;
}

int orbgpu_relocalize_batch_device(int n_queries, const orbgpu_reloc_query* d_queries, int n_cand,
                                   const orbgpu_reloc_candidate* d_cands, const orbgpu_reloc_frame* d_frames,
                                   const orbgpu_loop_keyframe* d_kfs, const orbgpu_loop_keyframe_search* d_kf_search,
                                   const int* d_match, int match_stride, const void* d_setup, int n_passes,
                                   int resume, void* d_state, orbgpu_relocalize_result* d_results,
                                   orbgpu_reloc_candidate_state* d_cand_states, int* d_rows, void* stream) {
    if (n_queries < 0 || n_cand < 0 || match_stride <= 0 || n_passes < 1 || (resume != 0 && resume != 1) ||
        (n_queries > 0 && (!d_queries || !d_cands || !d_frames || !d_kfs || !d_kf_search || !d_match || !d_setup ||
                           !d_state || !d_results || !d_cand_states || !d_rows)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if ((long long)n_queries * match_stride > 0x7fffffffLL / kRows || (long long)n_cand * match_stride > 0x7fffffffLL ||
        (long long)n_queries * kMaxHyp > 0x7fffffffLL / 4)
        return fail(ORBGPU_ERR_ARG, "n_queries or n_cand times match_stride overflows");
    if (n_queries == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const int nq = n_queries, S = match_stride;
    const Setup ws = carve_setup(const_cast<void*>(d_setup), n_cand, S, nullptr);
    const RState V = carve_state(d_state, nq, n_cand, S, nullptr);
    const dim3 grid(nq), block(kThreads);
#define RELOC_STAGE(K)                                                                                             \
    hipLaunchKernelGGL(reloc_stage_kernel<K>, grid, block, 0, s, d_queries, d_cands, d_frames, d_kfs, d_kf_search, S, n_cand, \
                       V, d_results, d_cand_states, d_rows);                                                         \
    ORB_HIP(hipGetLastError())
#define RELOC_POSEOPT()                                                                                            \
    if (int rc = orbgpu_pose_optimization_batch_device(nq, V.jobs, nq * S, V.Xw, V.obs, V.w, V.opt, V.outl, stream)) \
    return rc
#define RELOC_SEARCH() \
    if (int rc = orbgpu_search_by_projection_batch_device(nq, V.calls, S, V.pm, V.pn, stream)) return rc
    for (int pass = 0; pass < n_passes; ++pass) {
        hipLaunchKernelGGL(reloc_schedule_kernel, grid, block, 0, s, d_queries, n_cand, d_cands, d_frames, d_kfs,
                           d_kf_search, S, ws, pass == 0 ? resume : 1, V, d_results, d_rows);
        ORB_HIP(hipGetLastError());
        if (int rc = orbgpu_pnp_ransac_batch_device(nq, V.probs, kMaxHyp, n_cand * S, nq * kMaxHyp, ws.P3, ws.P2, ws.err,
                                                    V.samples, V.pnp_ws, V.pres, V.best_mask, V.refined_mask, stream))
            return rc;
        hipLaunchKernelGGL(reloc_after_pnp_kernel, grid, block, 0, s, d_queries, d_cands, d_frames, d_kfs, d_kf_search,
                           d_match, S, ws, V, d_results, d_rows);
        ORB_HIP(hipGetLastError());
        RELOC_POSEOPT();
        RELOC_STAGE(1);
        RELOC_SEARCH();
        RELOC_STAGE(2);
        RELOC_POSEOPT();
        RELOC_STAGE(3);
        RELOC_SEARCH();
        RELOC_STAGE(4);
        RELOC_POSEOPT();
        RELOC_STAGE(5);
    }
#undef RELOC_STAGE
#undef RELOC_POSEOPT
#undef RELOC_SEARCH
    return ORBGPU_OK;
}

}  // extern "C"
