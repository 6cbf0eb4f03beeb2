// loop_verify.hip -- the whole `while (nCandidates > 0 && !bMatch)` loop of
// LoopClosing::ComputeSim3 (src/LoopClosing.cpp:339-411), verification
// included (include/orbgpu_loop.h: orbgpu_compute_sim3_verified_batch_device).
// One *pass* takes every unfinished query to its next RANSAC return and
// verifies that Sim3; a pass is six launches on the caller's stream:
//
//   compute_sim3_resume_kernel  one 512-thread block per query: compute_sim3_kernel's
//                        windows (loop.hip; the layout, solve and score code is
//                        loop_device.h / sim3_device.h, shared) from the query's
//                        stored cursor, stream and solver states, up to the first
//                        return.  A return ends that iterate() call: the state
//                        stored is the one after exactly the consumed draws, the
//                        candidate that returned stays scheduled (a return never
//                        sets bNoMore, Sim3Solver.cpp:206-218) and the cursor is
//                        the next candidate of the same round.  A scheduled
//                        candidate whose iterations are used up gets an empty
//                        call: no draws, bNoMore, discarded.
//   verify_prep_kernel   vbInliers -> vpMapPointMatches (LoopClosing.cpp:370-378),
//                        SearchBySim3's vbAlreadyMatched1/2 as point flags
//                        (ORBmatcher.cpp:1282-1296) and the two SIM3_DIR calls
//                        ([sR21|t21] / [sR12|t12] with proj.cpp's arithmetic).
//   proj_kernel          (proj.hip) both directions of every verifying query;
//                        the other queries' calls have no points and no keypoints.
//   verify_gather_kernel the agreement check (:1472-1488) and OptimizeSim3's gathers
//                        (Optimizer.cpp:1284-1366) as an order-preserving
//                        compaction (ballot prefix sums, as sim3_setup_kernel),
//                        and the sim3opt job (n = 0 for the other queries).
//   sim3opt_kernel       (sim3opt.hip) both optimisations and both checks.
//   verify_decide_kernel removed correspondences out of the row, nIn >= 20,
//                        mg2oScw = gScm * Sim3(Rcw2, tcw2, 1.0) (:402-405).
//
// Nothing synchronises with the host; all values are written with plain stores.
#include "../../include/orbgpu_loop.h"
#include "host_common.h"
#include "loop_device.h"
#include "orbgpu_internal.h"
#include "sim3opt_device.h"

namespace orbgpu {

namespace {

using namespace loopdev;
namespace lm = orbgpu::lm;

constexpr int kVThreads = 256;  // the three verify kernels

struct QState {  // a query between passes
    int status;         // ORBGPU_SIM3_*
    int verify;         // this pass' RANSAC returned: candidate last_c is being verified
    int round, next_c;  // the schedule cursor: the next iterate() call is candidate next_c's in `round`
    int total;          // hypotheses consumed
    int verifications;
    int last_c;
    int pad;
    orbgpu_rand_state rng;
};

struct CState {  // a Sim3Solver between passes
    int n, max_its, its, best, live;
    Hyp hyp;     // the best hypothesis (mBestT12 and what its inlier flags are recomputed from)
};

struct VState {  // the opaque block, carved
    QState* q;
    CState* c;                 // kMaxC per query
    orbgpu_proj_call* calls;   // 2 per query: KF1's points into KF2, KF2's into KF1
    int* flags;                // one stride row per call
    int* pm;                   // the calls' per-point rows (vnMatch1, vnMatch2)
    int* pn;                   // and counts
    int* m;                    // vpMapPointMatches by KF1 slot: the KF2 slot or -1
    float *P1c, *P2c, *obs1, *obs2, *w1, *w2;  // the gathered correspondences, query q at q * stride
    int* gidx;                 // their KF1 slots
    orbgpu_sim3opt_job* jobs;
    orbgpu_sim3opt_result* opt;
    uint8_t* removed;
};

__host__ __device__ inline VState carve_state(void* base, int nq, int stride, size_t* bytes) {
    const size_t Q = (size_t)(nq > 0 ? nq : 1), S = (size_t)(stride > 0 ? stride : 1);
    char* p = static_cast<char*>(base);
    VState v;
    v.q = take<QState>(p, Q);
    v.c = take<CState>(p, Q * kMaxC);
    v.calls = take<orbgpu_proj_call>(p, 2 * Q);
    v.flags = take<int>(p, 2 * Q * S);
    v.pm = take<int>(p, 2 * Q * S);
    v.pn = take<int>(p, 2 * Q);
    v.m = take<int>(p, Q * S);
    v.P1c = take<float>(p, 3 * Q * S);
    v.P2c = take<float>(p, 3 * Q * S);
    v.obs1 = take<float>(p, 2 * Q * S);
    v.obs2 = take<float>(p, 2 * Q * S);
    v.w1 = take<float>(p, Q * S);
    v.w2 = take<float>(p, Q * S);
    v.gidx = take<int>(p, Q * S);
    v.jobs = take<orbgpu_sim3opt_job>(p, Q);
    v.opt = take<orbgpu_sim3opt_result>(p, Q);
    v.removed = take<uint8_t>(p, Q * S);
    if (bytes) *bytes = (size_t)(p - static_cast<char*>(base));
    return v;
}

// ------------------------------------------------------------------ the resumable RANSAC

__global__ __launch_bounds__(kQThreads) void compute_sim3_resume_kernel(
    const orbgpu_compute_sim3_query* __restrict__ queries, const orbgpu_sim3_candidate* __restrict__ cands,
    const orbgpu_loop_keyframe* __restrict__ kfs, int stride, Workspace ws, const int* __restrict__ n_corr,
    orbgpu_sim3_ransac_params prm, int resume, QState* __restrict__ qstates, CState* __restrict__ cstates,
    orbgpu_compute_sim3_verified_result* __restrict__ results, orbgpu_sim3_candidate_state* __restrict__ states) {
    __shared__ Hyp s_hyp[kWin];
    __shared__ Hyp s_best[kMaxC];
    __shared__ int s_slot_c[kWin], s_slot_r[kWin], s_trip[kWin][3], s_cnt[kWin];
    __shared__ unsigned long long s_pre_dead[kWin];  // candidates discarded by empty calls laid out just before the slot
    __shared__ unsigned char s_slot_last[kWin];      // the slot is the last iteration of its iterate() call
    __shared__ int c_n[kMaxC], c_max[kMaxC], c_its[kMaxC], c_best[kMaxC], c_sched[kMaxC];
    __shared__ int32_t s_r[31];
    __shared__ int32_t s_snap[31], s_gen[3 * kWin];  // as in compute_sim3_kernel: the window's start state and raw draws
    __shared__ int s_nslots, s_done, s_matched, s_round, s_total;
    __shared__ unsigned long long s_live;  // scheduled candidates: lane 0's, shared at the start and the end
    __shared__ float s_K[kMaxC][8];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    QState& S = qstates[q];
    CState* CS = cstates + (size_t)q * kMaxC;
    const int status = resume ? S.status : ORBGPU_SIM3_PENDING;  // read before any lane writes S
    __syncthreads();
    if (status != ORBGPU_SIM3_PENDING) {  // finished: the pass does nothing
        if (tid == 0) S.verify = 0;
        return;
    }
    const orbgpu_compute_sim3_query Q = queries[q];
    const int nc = min(Q.n_cand, kMaxC);
    const int c0 = Q.first_cand;
    const int ipc = prm.iterations_per_call;
    if (tid == 0) s_live = 0ull;
    __syncthreads();
    if (tid < nc) {
        const orbgpu_sim3_candidate cd = cands[c0 + tid];
        for (int k = 0; k < 4; ++k) {
            s_K[tid][k] = kfs[cd.kf1].K[k];
            s_K[tid][4 + k] = kfs[cd.kf2].K[k];
        }
        bool live;
        if (!resume) {  // Sim3Solver::SetRansacParameters (Sim3Solver.cpp:111-141)
            const int N = n_corr[c0 + tid];
            c_n[tid] = N;
            c_max[tid] = ransac_max_iterations(N, prm);
            c_its[tid] = 0;
            c_best[tid] = 0;
            // no solver (N < 0): discarded from the start.  A solver with N < minInliers stays scheduled
            // until its first iterate() call returns bNoMore at once (:151-156): an empty call, below
            live = N >= 0;
            float* hz = reinterpret_cast<float*>(&s_best[tid]);
            for (int k = 0; k < (int)(sizeof(Hyp) / 4); ++k) hz[k] = 0.f;
        } else {
            const CState& C = CS[tid];
            c_n[tid] = C.n;
            c_max[tid] = C.max_its;
            c_its[tid] = C.its;
            c_best[tid] = C.best;
            live = C.live != 0;
            s_best[tid] = C.hyp;
        }
        c_sched[tid] = c_its[tid];  // between passes no call is under way
        if (live) atomicOr(&s_live, 1ull << tid);
    }
    if (tid == 0) {
        const orbgpu_rand_state& R0 = resume ? S.rng : Q.rng;
        for (int k = 0; k < 31; ++k) s_r[k] = R0.r[k];
        s_done = 0;
        s_matched = -1;
        s_round = -1;
        s_total = resume ? S.total : 0;
        if (!resume) {  // every word of the result starts at zero
            int* w = reinterpret_cast<int*>(&results[q]);
            for (int k = 0; k < (int)(sizeof(orbgpu_compute_sim3_verified_result) / 4); ++k) w[k] = 0;
            results[q].matched = -1;
            results[q].round = -1;
            results[q].last_cand = -1;
        }
    }
    __syncthreads();
    // lane 0's stream indices, schedule cursor and scheduled set
    int rf = resume ? S.rng.f : Q.rng.f, rb = resume ? S.rng.b : Q.rng.b;
    int snap_f = rf, snap_b = rb, snap_total = s_total;
    int cur_round = resume ? S.round : 0, cur_c = resume ? S.next_c : 0, cur_j = 0;
    unsigned long long live = s_live, live_snap = live;
    bool sched_end = false;
    int win = 32;  // windows grow 32, 64, .., kWin as in compute_sim3_kernel
    while (true) {
        if (tid == 0) {  // lay out the next window in the reference's order
            for (int k = 0; k < 31; ++k) s_snap[k] = s_r[k];
            snap_f = rf;
            snap_b = rb;
            snap_total = s_total;
            live_snap = live;  // exact: everything laid out before this window was consumed
            unsigned long long pending_dead = 0ull;
            int n = 0;
            while (n < win && !sched_end) {
                if (cur_c == nc) {  // next round of `while (nCandidates > 0 && !bMatch)`
                    if (!live) {
                        sched_end = true;
                        break;
                    }
                    cur_c = 0;
                    ++cur_round;
                }
                const int c = cur_c;
                if (!((live >> c) & 1ull)) {
                    ++cur_c;
                    continue;
                }
                // iterations of this iterate() call
                const int k = c_n[c] < prm.min_inliers ? 0 : min(ipc, c_max[c] - c_sched[c]);
                if (k <= 0) {  // an empty call (N < minInliers, or after a return on the last iteration): bNoMore, no draws
                    live &= ~(1ull << c);
                    pending_dead |= 1ull << c;
                    ++cur_c;
                    continue;
                }
                for (; cur_j < k && n < win; ++cur_j, ++n) {
                    draw_triplet(c_n[c], s_r, rf, rb, &s_gen[3 * n], s_trip[n]);
                    s_slot_c[n] = c;
                    s_slot_r[n] = cur_round;
                    s_pre_dead[n] = pending_dead;
                    pending_dead = 0ull;
                    s_slot_last[n] = cur_j == k - 1 ? 1 : 0;
                }
                if (cur_j == k) {  // the call is laid out completely
                    cur_j = 0;
                    c_sched[c] += k;
                    if (c_sched[c] >= c_max[c]) live &= ~(1ull << c);  // bNoMore -> vbDiscarded (:349-353)
                    ++cur_c;
                }
            }
            s_nslots = n;
        }
        __syncthreads();
        const int ns = s_nslots;
        if (ns == 0) break;
        if (tid < ns) {  // ComputeSim3 for one hypothesis
            const int c = s_slot_c[tid];
            const size_t o = (size_t)(c0 + c) * stride;
            float A[3][3], B[3][3];
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < 3; ++i) {
                    A[k][i] = ws.X1[3 * (o + s_trip[tid][k]) + i];
                    B[k][i] = ws.X2[3 * (o + s_trip[tid][k]) + i];
                }
            compute_sim3(A, B, prm.fix_scale != 0, s_hyp[tid]);
        }
        __syncthreads();
        for (int p = wave; 2 * p < ns; p += kQThreads / 64) {  // CheckInliers, a pair of hypotheses per wave
            const int h0 = 2 * p, h1 = 2 * p + 1;
            const bool both = h1 < ns && s_slot_c[h1] == s_slot_c[h0];  // wave-uniform
            auto check = [&](int h, int hb, bool two) {
                const int cc = s_slot_c[h];
                int cnt, cntb;
                score_pair(ws, (size_t)(c0 + cc) * stride, c_n[cc], s_K[cc], s_K[cc] + 4, s_hyp[h], s_hyp[hb], two, lane,
                           cnt, cntb);
                if (lane == 0) {
                    s_cnt[h] = cnt;
                    if (two) s_cnt[hb] = cntb;
                }
            };
            if (both) {
                check(h0, h1, true);
            } else {
                check(h0, h0, false);
                if (h1 < ns) check(h1, h1, false);
            }
        }
        __syncthreads();
        if (tid == 0) {  // the reference's acceptance, in stream order (Sim3Solver.cpp:199-212)
            unsigned long long x_live = live_snap;  // the scheduled set after exactly the consumed calls
            for (int h = 0; h < ns; ++h) {
                const int c = s_slot_c[h], cnt = s_cnt[h];
                x_live &= ~s_pre_dead[h];
                ++c_its[c];
                ++s_total;
                if (cnt >= c_best[c]) {
                    c_best[c] = cnt;
                    s_best[c] = s_hyp[h];
                    if (cnt > prm.min_inliers) {
                        // the return ends this iterate() call without bNoMore: c stays scheduled, and the
                        // hypotheses laid out past h are dropped with their draws
                        s_matched = c;
                        s_round = s_slot_r[h];
                        s_done = 1;
                        live = x_live;
                        cur_round = s_slot_r[h];
                        cur_c = c + 1;
                        cur_j = 0;
                        break;
                    }
                }
                if (s_slot_last[h] && c_its[c] >= c_max[c]) x_live &= ~(1ull << c);
            }
        }
        __syncthreads();
        if (s_done) break;
        win = min(2 * win, kWin);
    }
    __syncthreads();
    if (tid == 0) s_live = live;
    __syncthreads();
    const int mc = s_matched;
    const unsigned long long live_out = s_live;
    if (tid < nc) {
        const int lv = (int)((live_out >> tid) & 1ull);
        CState& C = CS[tid];
        C.n = c_n[tid];
        C.max_its = c_max[tid];
        C.its = c_its[tid];
        C.best = c_best[tid];
        C.live = lv;
        C.hyp = s_best[tid];
        orbgpu_sim3_candidate_state& T = states[c0 + tid];
        T.n = c_n[tid];
        T.max_iterations = c_max[tid];
        T.iterations = c_its[tid];
        T.best_inliers = c_best[tid];
        T.discarded = lv ? 0 : 1;
        T.pad = 0;
    }
    if (tid == 0) {
        orbgpu_compute_sim3_verified_result& R = results[q];
        // the stream after exactly the consumed draws, as compute_sim3_kernel rebuilds it
        const int K = 3 * (s_total - snap_total);
        for (int j = max(0, K - 31); j < K; ++j) s_snap[(snap_f + j) % 31] = s_gen[j];
        for (int k = 0; k < 31; ++k) S.rng.r[k] = R.rng_after.r[k] = s_snap[k];
        S.rng.f = R.rng_after.f = (snap_f + K) % 31;
        S.rng.b = R.rng_after.b = (snap_b + K) % 31;
        S.total = s_total;
        R.hypotheses = s_total;
        R.draws = 3 * s_total;
        S.round = cur_round;
        S.next_c = cur_c;
        S.pad = 0;
        if (!resume) S.verifications = 0;
        if (mc >= 0) {
            S.status = ORBGPU_SIM3_PENDING;
            S.verify = 1;
            S.last_c = mc;
            R.status = ORBGPU_SIM3_PENDING;
            R.round = s_round;
            R.last_cand = mc;
            R.n_inliers = c_best[mc];
            const Hyp& H = s_best[mc];
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) R.T12[4 * i + j] = H.sR[3 * i + j];
                R.T12[4 * i + 3] = H.t[i];
                R.t12[i] = H.t[i];
            }
            R.T12[12] = R.T12[13] = R.T12[14] = 0.f;
            R.T12[15] = 1.f;
            for (int k = 0; k < 9; ++k) R.R12[k] = H.R[k];
            R.s12 = H.s;
        } else {  // no candidate is scheduled any more
            S.status = ORBGPU_SIM3_NO_MATCH;
            S.verify = 0;
            if (!resume) S.last_c = -1;
            R.status = ORBGPU_SIM3_NO_MATCH;
            R.matched = -1;
            R.round = -1;
        }
    }
}

// ------------------------------------------------------------------ the verification

__global__ __launch_bounds__(kVThreads) void verify_prep_kernel(
    const orbgpu_compute_sim3_query* __restrict__ queries, const orbgpu_sim3_candidate* __restrict__ cands,
    const orbgpu_loop_keyframe* __restrict__ kfs, const orbgpu_loop_keyframe_search* __restrict__ kss,
    const int* __restrict__ match12, int stride, Workspace ws, float th_search, VState V, int* __restrict__ rows) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const QState& S = V.q[q];
    orbgpu_proj_call* calls = V.calls + 2 * (size_t)q;
    if (!S.verify) {
        if (tid < 2) idle_call(calls[tid], ORBGPU_PROJ_SIM3_DIR);
        return;
    }
    const int c = S.last_c, gc = queries[q].first_cand + c;
    const orbgpu_sim3_candidate cd = cands[gc];
    const orbgpu_loop_keyframe& K1 = kfs[cd.kf1];
    const orbgpu_loop_keyframe& K2 = kfs[cd.kf2];
    const CState& C = V.c[(size_t)q * kMaxC + c];
    const int n1 = min(K1.n, stride), n2 = min(K2.n, stride);
    int* m = V.m + (size_t)q * stride;
    int* vb = rows + (size_t)q * 3 * stride;
    int* f1 = V.flags + (size_t)(2 * q) * stride;
    int* f2 = V.flags + (size_t)(2 * q + 1) * stride;
    for (int i = tid; i < stride; i += kVThreads) {
        m[i] = -1;
        vb[i] = 0;
    }
    __syncthreads();
    {  // vbInliers of the returned hypothesis; vpMapPointMatches[i1] = vvpMapPointMatches[c][i1] there
        const size_t o = (size_t)gc * stride;
        const int* row = match12 + o;
        const Hyp H = C.hyp;
        for (int j = tid; j < C.n; j += kVThreads) {
            if (is_inlier_pre(H, K1.K, K2.K, ws.X1 + 3 * (o + j), ws.X2 + 3 * (o + j), ws.P1[o + j], ws.P2[o + j],
                              ws.e1[o + j], ws.e2[o + j])) {
                const int i1 = ws.idx1[o + j];
                vb[i1] = 1;
                m[i1] = row[i1];
            }
        }
    }
    __syncthreads();
    // vbAlreadyMatched1 / vbAlreadyMatched2 (ORBmatcher.cpp:1282-1296) folded into the point flags
    for (int i = tid; i < stride; i += kVThreads) {
        f1[i] = (i < n1 && K1.mp_valid[i] && m[i] < 0) ? ORBGPU_PT_VALID : 0;
        f2[i] = (i < n2 && K2.mp_valid[i]) ? ORBGPU_PT_VALID : 0;
    }
    __syncthreads();
    for (int i = tid; i < n1; i += kVThreads) {
        const int i2 = m[i];
        if (i2 >= 0 && i2 < n2) f2[i2] = 0;
    }
    if (tid < 2) {
        const int dir = tid;
        const Hyp& H = C.hyp;
        // sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (ORBmatcher.cpp:1272-1274), with the
        // arithmetic of orbgpu_search_by_sim3 (proj.cpp)
        float sR12[9], sR21[9], t21[3];
        const double inv = 1.0 / (double)H.s;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                sR12[3 * i + j] = (float)((double)H.R[3 * i + j] * (double)H.s);
                sR21[3 * i + j] = (float)((double)H.R[3 * j + i] * inv);
            }
        for (int i = 0; i < 3; ++i)
            t21[i] = -(float)((double)sR21[3 * i] * H.t[0] + (double)sR21[3 * i + 1] * H.t[1] +
                              (double)sR21[3 * i + 2] * H.t[2]);
        const orbgpu_loop_keyframe_search& A = kss[dir == 0 ? cd.kf1 : cd.kf2];  // the points' keyframe
        const orbgpu_loop_keyframe_search& B = kss[dir == 0 ? cd.kf2 : cd.kf1];  // the keyframe searched
        const orbgpu_loop_keyframe& KA = dir == 0 ? K1 : K2;
        const orbgpu_proj_target& T1 = kss[cd.kf1].target;
        orbgpu_proj_call& k = calls[dir];
        idle_call(k, ORBGPU_PROJ_SIM3_DIR);
        k.th = th_search;
        k.target = B.target;
        k.target.u_right = nullptr;
        k.target.occupied = nullptr;
        k.target.fx = T1.fx;  // pKF1's intrinsics both ways (:1257-1260)
        k.target.fy = T1.fy;
        k.target.cx = T1.cx;
        k.target.cy = T1.cy;
        const float* R = dir == 0 ? sR21 : sR12;
        const float* t = dir == 0 ? t21 : H.t;
        for (int i = 0; i < 16; ++i) k.target.Tcw[i] = (i == 15) ? 1.f : 0.f;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) k.target.Tcw[4 * i + j] = R[3 * i + j];
            k.target.Tcw[4 * i + 3] = t[i];
        }
        for (int i = 0; i < 16; ++i) k.last_Tcw[i] = A.target.Tcw[i];
        k.points.n = KA.n;
        k.points.flags = dir == 0 ? f1 : f2;
        k.points.pos = KA.mp_world;
        k.points.desc = A.mp_desc;
        k.points.min_dist = A.mp_min_dist;
        k.points.max_dist = A.mp_max_dist;
    }
}

__global__ __launch_bounds__(kVThreads) void verify_gather_kernel(
    const orbgpu_compute_sim3_query* __restrict__ queries, const orbgpu_sim3_candidate* __restrict__ cands,
    const orbgpu_loop_keyframe* __restrict__ kfs, const orbgpu_loop_keyframe_search* __restrict__ kss, int stride,
    float th2, int fix_scale, VState V, orbgpu_compute_sim3_verified_result* __restrict__ results,
    int* __restrict__ rows) {
    __shared__ int s_wave[kVThreads / 64];
    __shared__ int s_found;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    QState& S = V.q[q];
    orbgpu_sim3opt_job& J = V.jobs[q];
    const int verify = S.verify;
    const int nm0 = V.pn[2 * q], nm1 = V.pn[2 * q + 1];
    if (tid == 0) s_found = 0;
    __syncthreads();
    if (!verify || nm0 < 0 || nm1 < 0) {
        if (tid == 0) {
            int* w = reinterpret_cast<int*>(&J);
            for (int k = 0; k < (int)(sizeof(orbgpu_sim3opt_job) / 4); ++k) w[k] = 0;
            J.offset = q * stride;
            J.q12[3] = 1.0;
            J.s12 = 1.0;
            if (verify) {  // a keyframe over the projection matcher's capacity: the query ends, nothing truncated
                S.status = ORBGPU_SIM3_CAPACITY;
                S.verify = 0;
                results[q].status = ORBGPU_SIM3_CAPACITY;
            }
        }
        return;
    }
    const int c = S.last_c, gc = queries[q].first_cand + c;
    const orbgpu_sim3_candidate cd = cands[gc];
    const orbgpu_loop_keyframe& K1 = kfs[cd.kf1];
    const orbgpu_loop_keyframe& K2 = kfs[cd.kf2];
    const orbgpu_loop_keyframe_search& A1 = kss[cd.kf1];
    const orbgpu_loop_keyframe_search& A2 = kss[cd.kf2];
    // the two tables describe the same keyframes; the smaller count bounds every index
    const int n1 = min(min(K1.n, A1.target.n), stride), n2 = min(min(K2.n, A2.target.n), stride);
    int* m = V.m + (size_t)q * stride;
    int* agreed = rows + ((size_t)q * 3 + 1) * stride;
    const int* v1 = V.pm + (size_t)(2 * q) * stride;      // vnMatch1
    const int* v2 = V.pm + (size_t)(2 * q + 1) * stride;  // vnMatch2
    int found = 0;
    for (int i1 = tid; i1 < stride; i1 += kVThreads) {  // check agreement (ORBmatcher.cpp:1472-1488)
        int a = -1;
        if (i1 < n1) {
            const int idx2 = v1[i1];
            if (idx2 >= 0 && idx2 < n2 && v2[idx2] == i1) a = idx2;
        }
        agreed[i1] = a;
        if (a >= 0) {
            m[i1] = a;
            ++found;
        }
    }
    if (found) atomicAdd(&s_found, found);
    __syncthreads();
    // OptimizeSim3's gathers (Optimizer.cpp:1284-1366) in ascending i1
    const size_t o = (size_t)q * stride;
    int base = 0;
    for (int s = 0; s < n1; s += kVThreads) {
        const int i1 = s + tid;
        int i2 = -1;
        if (i1 < n1) {
            i2 = m[i1];
            if (i2 >= n2 || (i2 >= 0 && !(K1.mp_valid[i1] && K2.mp_valid[i2]))) i2 = -1;
        }
        const bool ok = i2 >= 0;
        const unsigned long long bm = __ballot(ok);
        if (lane == 0) s_wave[wave] = __popcll(bm);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (ok) {
            const size_t j = o + before + (int)__popcll(bm & ((1ull << lane) - 1));
            float Xw[3];
            for (int k = 0; k < 3; ++k) Xw[k] = K1.mp_world[3 * (size_t)i1 + k];
            for (int k = 0; k < 3; ++k) V.P1c[3 * j + k] = gemv_row(&K1.Rcw[3 * k], Xw) + K1.tcw[k];
            for (int k = 0; k < 3; ++k) Xw[k] = K2.mp_world[3 * (size_t)i2 + k];
            for (int k = 0; k < 3; ++k) V.P2c[3 * j + k] = gemv_row(&K2.Rcw[3 * k], Xw) + K2.tcw[k];
            const orbgpu_keypoint kp1 = A1.target.kps[i1], kp2 = A2.target.kps[i2];
            V.obs1[2 * j] = kp1.x;
            V.obs1[2 * j + 1] = kp1.y;
            V.obs2[2 * j] = kp2.x;
            V.obs2[2 * j + 1] = kp2.y;
            V.w1[j] = A1.inv_level_sigma2[kp1.octave & 15];
            V.w2[j] = A2.inv_level_sigma2[kp2.octave & 15];
            V.gidx[j] = i1;
        }
        for (int w = 0; w < kVThreads / 64; ++w) base += s_wave[w];
        __syncthreads();
    }
    if (tid == 0) {
        const CState& C = V.c[(size_t)q * kMaxC + c];
        // gScm = Sim3(Converter::toMatrix3d(R), toVector3d(t), s) (LoopClosing.cpp:390): Quaterniond(Matrix3d)
        double R[9], qd[4];
        for (int k = 0; k < 9; ++k) R[k] = (double)C.hyp.R[k];
        lm::quat_from_R(R, qd);
        J.n = base;
        J.offset = q * stride;
        for (int k = 0; k < 4; ++k) J.q12[k] = qd[k];
        for (int k = 0; k < 3; ++k) J.t12[k] = (double)C.hyp.t[k];
        J.s12 = (double)C.hyp.s;
        for (int k = 0; k < 4; ++k) {
            J.K1[k] = K1.K[k];
            J.K2[k] = K2.K[k];
        }
        J.th2 = th2;
        J.fix_scale = fix_scale;
        results[q].n_found = s_found;
        results[q].n_gathered = base;
    }
}

__global__ __launch_bounds__(kVThreads) void verify_decide_kernel(
    const orbgpu_compute_sim3_query* __restrict__ queries, const orbgpu_sim3_candidate* __restrict__ cands,
    const orbgpu_loop_keyframe* __restrict__ kfs, int stride, int min_opt_inliers, VState V,
    orbgpu_compute_sim3_verified_result* __restrict__ results, int* __restrict__ rows) {
    const int q = blockIdx.x, tid = threadIdx.x;
    QState& S = V.q[q];
    const int verify = S.verify;
    __syncthreads();
    if (!verify) return;
    int* m = V.m + (size_t)q * stride;
    int* out = rows + ((size_t)q * 3 + 2) * stride;
    const size_t o = (size_t)q * stride;
    const orbgpu_sim3opt_result& O = V.opt[q];
    const int n = V.jobs[q].n;
    for (int j = tid; j < n; j += kVThreads)  // vpMatches1[idx] = NULL (Optimizer.cpp:1389, :1421)
        if (V.removed[o + j]) m[V.gidx[o + j]] = -1;
    __syncthreads();
    for (int i = tid; i < stride; i += kVThreads) out[i] = m[i];
    if (tid == 0) {
        orbgpu_compute_sim3_verified_result& R = results[q];
        const int c = S.last_c;
        S.verifications += 1;
        S.verify = 0;
        R.verifications = S.verifications;
        R.opt = O;
        if (O.n_in >= min_opt_inliers) {  // LoopClosing.cpp:396-409
            const orbgpu_loop_keyframe& K2 = kfs[cands[queries[q].first_cand + c].kf2];
            sim3opt::Sim3 gScm, gSmw, gScw;
            for (int k = 0; k < 4; ++k) gScm.q[k] = O.q12[k];
            for (int k = 0; k < 3; ++k) gScm.t[k] = O.t12[k];
            gScm.s = O.s12;
            double Rm[9];
            for (int k = 0; k < 9; ++k) Rm[k] = (double)K2.Rcw[k];
            lm::quat_from_R(Rm, gSmw.q);
            for (int k = 0; k < 3; ++k) gSmw.t[k] = (double)K2.tcw[k];
            gSmw.s = 1.0;
            sim3opt::sim3_mul(gScm, gSmw, gScw);
            for (int k = 0; k < 4; ++k) R.Scw_q[k] = gScw.q[k];
            for (int k = 0; k < 3; ++k) R.Scw_t[k] = gScw.t[k];
            R.Scw_s = gScw.s;
            lm::write_T16(R.Scw_q, R.Scw_t, R.Scw_s, R.Scw);
            R.matched = c;
            R.status = ORBGPU_SIM3_MATCHED;
            S.status = ORBGPU_SIM3_MATCHED;
        }
    }
}

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

size_t orbgpu_compute_sim3_verified_workspace_bytes(int n_queries, int match_stride) {
    size_t bytes = 0;
    carve_state(nullptr, n_queries, match_stride, &bytes);
    return bytes;
}

int orbgpu_compute_sim3_verified_batch_device(
    int n_queries, const orbgpu_compute_sim3_query* d_queries, int n_cand, const orbgpu_sim3_candidate* d_cands,
    const orbgpu_loop_keyframe* d_kfs, const orbgpu_loop_keyframe_search* d_kf_search, const int* d_match12,
    int match_stride, const void* d_workspace, const int* d_n_corr, orbgpu_sim3_ransac_params params, float th_search,
    float th2, int min_opt_inliers, int n_passes, int resume, void* d_state,
    orbgpu_compute_sim3_verified_result* d_results, orbgpu_sim3_candidate_state* d_cand_states, int* d_rows,
    void* stream) {
    if (n_queries < 0 || n_cand < 0 || match_stride <= 0 || params.iterations_per_call < 1 || params.max_iterations < 1 ||
        params.min_inliers < 0 || !(params.probability > 0.0 && params.probability < 1.0) || !(th_search > 0.f) ||
        !(th2 > 0.f) || min_opt_inliers < 0 || n_passes < 1 || (resume != 0 && resume != 1) ||
        (n_queries > 0 && (!d_queries || !d_cands || !d_kfs || !d_kf_search || !d_match12 || !d_workspace || !d_n_corr ||
                           !d_state || !d_results || !d_cand_states || !d_rows)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if ((long long)n_queries * match_stride > 0x7fffffffLL) return fail(ORBGPU_ERR_ARG, "n_queries * match_stride overflows");
    if (n_queries == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const Workspace ws = carve(const_cast<void*>(d_workspace), n_cand, match_stride);
    const VState V = carve_state(d_state, n_queries, match_stride, nullptr);
    for (int pass = 0; pass < n_passes; ++pass) {
        hipLaunchKernelGGL(compute_sim3_resume_kernel, dim3(n_queries), dim3(kQThreads), 0, s, d_queries, d_cands, d_kfs,
                           match_stride, ws, d_n_corr, params, pass == 0 ? resume : 1, V.q, V.c, d_results, d_cand_states);
        ORB_HIP(hipGetLastError());
        hipLaunchKernelGGL(verify_prep_kernel, dim3(n_queries), dim3(kVThreads), 0, s, d_queries, d_cands, d_kfs,
                           d_kf_search, d_match12, match_stride, ws, th_search, V, d_rows);
        ORB_HIP(hipGetLastError());
        if (int rc = orbgpu_search_by_projection_batch_device(2 * n_queries, V.calls, match_stride, V.pm, V.pn, stream))
            return rc;
        hipLaunchKernelGGL(verify_gather_kernel, dim3(n_queries), dim3(kVThreads), 0, s, d_queries, d_cands, d_kfs,
                           d_kf_search, match_stride, th2, params.fix_scale, V, d_results, d_rows);
        ORB_HIP(hipGetLastError());
        if (int rc = orbgpu_optimize_sim3_batch_device(n_queries, V.jobs, n_queries * match_stride, V.P1c, V.P2c, V.obs1,
                                                       V.obs2, V.w1, V.w2, V.opt, V.removed, stream))
            return rc;
        hipLaunchKernelGGL(verify_decide_kernel, dim3(n_queries), dim3(kVThreads), 0, s, d_queries, d_cands, d_kfs,
                           match_stride, min_opt_inliers, V, d_results, d_rows);
        ORB_HIP(hipGetLastError());
    }
    return ORBGPU_OK;
}

}  // extern "C"
