// track.hip -- Tracking's per-frame chain on the device (include/orbgpu_track.h):
// TrackWithMotionModel / TrackReferenceKeyFrame, SearchLocalPoints + TrackLocalMap
// and UpdateLastFrame's visual-odometry points, each batched over independent
// frames.  Every stage is one workgroup per frame on the caller's stream:
//
//  orbgpu_track_initial_batch_device (src/Tracking.cpp:977-1025, :1126-1198)
//    1 initial_begin_kernel    the job's checks, an all-NULL occupancy (:1141), the
//                              LAST_FRAME call with ORBmatcher(0.9, true) and th
//    2 proj                    orbgpu_search_by_projection_batch_device, unchanged
//    3 initial_retry_kernel    nmatches < 20 -> the same call with 2*th on a NULL row
//                              (:1156-1160), else an idle call
//    4 proj
//    5 initial_gather_kernel   nmatches < 20 (BoW: < 15) -> FEW_MATCHES; row entries >= 0
//                              become mvpMapPoints; PoseOptimization's gather
//    6 poseopt                 orbgpu_pose_optimization_batch_device, unchanged
//    7 initial_cull_kernel     the cull of :1172-1189 / :1005-1022 and the decision
//
//  orbgpu_track_local_map_batch_device (:1210-1264, :1496-1562)
//    1 local_begin_kernel      held bad points nulled, the others seen (:1501-1520);
//                              isInFrustum(., 0.5) of the local points neither seen nor
//                              flagged ORBGPU_PT_LAST_SEEN (call 1's culled, :1531) against the
//                              pose read from HBM, nToMatch (:1526-1545); the occupancy
//                              and the LOCAL call with ORBmatcher(0.8) and th
//    2 proj
//    3 local_gather_kernel     the matches enter mvpMapPoints; the gather
//    4 poseopt
//    5 local_decide_kernel     mnMatchesInliers, the stereo cull, the decision (:1230-1263)
//
//  orbgpu_update_last_frame_batch_device (:1053-1113): one kernel, a rank
//  selection over (z, i) in LDS.
//
// A frame that is not in a stage hands that stage an empty job (n = 0) or an
// idle call.  Nothing synchronises with the host; all values are written with
// plain stores.  proj.hip, poseopt.hip and reloc.hip are untouched: the few
// float helpers below restate proj.hip's (same expressions, same flags, so the
// same bits).
#include "../../include/orbgpu_track.h"
#include "host_common.h"
#include "ransac_device.h"

namespace orbgpu {

namespace {

using namespace ransacdev;

constexpr int kThreads = 256;
constexpr int kMaxKps = 4096;  // proj_kernel's keypoint capacity
constexpr int kPending = -1;   // a frame still in the chain

// ------------------------------------------------------------------ shared pieces

__device__ __forceinline__ void zero_words(void* p, size_t bytes) {
    int* w = reinterpret_cast<int*>(p);
    for (int k = 0; k < (int)(bytes / 4); ++k) w[k] = 0;
}

__device__ __forceinline__ void empty_job(orbgpu_poseopt_job& J, int offset) {
    zero_words(&J, sizeof(J));
    J.offset = offset;
}

// what PoseOptimization reads of one frame (Optimizer.cpp:317-392): the keypoints with a MapPoint,
// ascending; mp[j] indexes `pos`
struct Gather {
    orbgpu_poseopt_job* job;
    float *Xw, *obs, *w;  // already offset to the frame's range
    int* gidx;
};

__device__ __forceinline__ void gather_job(const orbgpu_reloc_frame& F, int nf, const int* mp, const float* pos,
                                           const float* Tcw, int offset, const Gather& G, int* s_wave) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const orbgpu_proj_target& T = F.target;
    int base = 0;
    for (int s = 0; s < nf; s += kThreads) {
        const int j = s + tid;
        const int p = j < nf ? mp[j] : -1;
        const bool ok = p >= 0;
        const int i = compact_slot(ok, lane, wave, s_wave, base);
        if (ok) {
            const orbgpu_keypoint kp = T.kps[j];
            for (int k = 0; k < 3; ++k) G.Xw[3 * (size_t)i + k] = pos[3 * (size_t)p + k];
            G.obs[3 * (size_t)i] = kp.x;
            G.obs[3 * (size_t)i + 1] = kp.y;
            G.obs[3 * (size_t)i + 2] = T.u_right ? T.u_right[j] : -1.f;
            G.w[i] = F.inv_level_sigma2[kp.octave & 15];
            G.gidx[i] = j;
        }
        compact_advance<kThreads>(s_wave, base);
        __syncthreads();
    }
    if (tid == 0) {
        orbgpu_poseopt_job& J = *G.job;
        empty_job(J, offset);
        J.n = base;
        for (int k = 0; k < 12; ++k) J.Tcw0[k] = Tcw[k];
        J.fx = T.fx;
        J.fy = T.fy;
        J.cx = T.cx;
        J.cy = T.cy;
        J.bf = T.bf;
    }
}

__device__ __forceinline__ void copy_opt(orbgpu_poseopt_result& dst, const orbgpu_poseopt_result& src) {
    const int* s = reinterpret_cast<const int*>(&src);
    int* d = reinterpret_cast<int*>(&dst);
    for (int k = 0; k < (int)(sizeof(orbgpu_poseopt_result) / 4); ++k) d[k] = s[k];
}

// ------------------------------------------------------------------ 1. the initial pose

struct IFrame {  // a frame between the stages
    int status;  // kPending or ORBGPU_TRACK_*
    int nf;      // the frame's keypoints
    int np;      // the point table's entries
    int searches;
    int n1;      // the first search's return
    int nm;      // nmatches before the cull
    int pad[2];
};

struct IWork {  // the opaque block, carved
    IFrame* st;
    int* mp;         // mvpMapPoints by frame keypoint: the table index or -1
    uint8_t* occ;    // all NULL (:1141, :1158); never written after the first stage
    int* pm[2];      // the two searches' rows and counts
    int* pn[2];
    orbgpu_proj_call* calls;
    orbgpu_poseopt_job* jobs;
    orbgpu_poseopt_result* opt;
    float *Xw, *obs, *w;
    int* gidx;
    uint8_t* outl;
};

inline IWork carve_initial(void* base, int n, int stride, size_t* bytes) {
    const size_t N = (size_t)(n > 0 ? n : 1), S = (size_t)(stride > 0 ? stride : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    IWork v;
    v.st = take<IFrame>(p, N);
    v.mp = take<int>(p, N * S);
    v.occ = take<uint8_t>(p, N * S);
    for (int k = 0; k < 2; ++k) {
        v.pm[k] = take<int>(p, N * S);
        v.pn[k] = take<int>(p, N);
    }
    v.calls = take<orbgpu_proj_call>(p, N);
    v.jobs = take<orbgpu_poseopt_job>(p, N);
    v.opt = take<orbgpu_poseopt_result>(p, N);
    v.Xw = take<float>(p, 3 * N * S);
    v.obs = take<float>(p, 3 * N * S);
    v.w = take<float>(p, N * S);
    v.gidx = take<int>(p, N * S);
    v.outl = take<uint8_t>(p, N * S);
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return v;
}

__global__ __launch_bounds__(kThreads) void initial_begin_kernel(const orbgpu_track_initial_job* __restrict__ jobs,
                                                                 int n_frames,
                                                                 const orbgpu_reloc_frame* __restrict__ frames,
                                                                 int stride, IWork V,
                                                                 orbgpu_track_initial_result* __restrict__ results,
                                                                 int* __restrict__ rows) {
    const int k = blockIdx.x, tid = threadIdx.x;
    const orbgpu_track_initial_job& J = jobs[k];
    const size_t o = (size_t)k * stride;
    int* rw = rows + (size_t)k * ORBGPU_TRACK_INITIAL_ROWS * stride;
    for (int i = tid; i < ORBGPU_TRACK_INITIAL_ROWS * stride; i += kThreads) rw[i] = -1;
    for (int i = tid; i < stride; i += kThreads) {
        V.mp[o + i] = -1;
        V.occ[o + i] = 0;
    }
    if (tid != 0) return;
    orbgpu_track_initial_result& R = results[k];
    zero_words(&R, sizeof(R));
    R.nsearch[0] = R.nsearch[1] = -1;
    IFrame& S = V.st[k];
    zero_words(&S, sizeof(S));
    orbgpu_proj_call& C = V.calls[k];
    idle_call(C, ORBGPU_PROJ_LAST_FRAME);
    empty_job(V.jobs[k], k * stride);
    int status = kPending;
    const bool motion = J.mode == ORBGPU_TRACK_MOTION;
    if ((!motion && J.mode != ORBGPU_TRACK_REFERENCE) || J.frame < 0 || J.frame >= n_frames || J.points.n < 0 ||
        (!motion && (!J.bow_row || !J.bow_nmatches))) {
        status = ORBGPU_TRACK_BAD_JOB;
    } else {
        const orbgpu_reloc_frame& F = frames[J.frame];
        const int nf = F.target.n;
        if (nf < 0 || nf > min(stride, kMaxKps)) {
            status = ORBGPU_TRACK_CAPACITY;
        } else {
            S.nf = nf;
            S.np = J.points.n;
            if (motion) {  // matcher.SearchByProjection(mCurrentFrame, mLastFrame, th, bMono) (:1152)
                C.check_ori = 1;
                C.nnratio = 0.9f;
                C.th = J.th;
                C.mono = J.mono != 0;
                for (int i = 0; i < 16; ++i) C.last_Tcw[i] = J.last_Tcw[i];
                C.target = F.target;
                C.target.occupied = V.occ + o;
                for (int i = 0; i < 16; ++i) C.target.Tcw[i] = J.Tcw_init[i];
                C.points = J.points;
            }
        }
    }
    S.status = status;
    R.status = status == kPending ? ORBGPU_TRACK_OK : status;
}

__global__ __launch_bounds__(64) void initial_retry_kernel(const orbgpu_track_initial_job* __restrict__ jobs, IWork V,
                                                           orbgpu_track_initial_result* __restrict__ results) {
    const int k = blockIdx.x;
    if (threadIdx.x != 0) return;
    IFrame& S = V.st[k];
    orbgpu_proj_call& C = V.calls[k];
    bool again = false;
    if (S.status == kPending && jobs[k].mode == ORBGPU_TRACK_MOTION) {
        const int n1 = V.pn[0][k];
        S.n1 = n1;
        S.searches = 1;
        results[k].nsearch[0] = n1;
        results[k].searches = 1;
        if (n1 < 0) {  // over the matcher's capacity after all: the frame ends, nothing truncated
            S.status = results[k].status = ORBGPU_TRACK_CAPACITY;
        } else if (n1 < ORBGPU_TRACK_MIN_MATCHES) {  // :1156-1160; the occupancy is still all NULL
            C.th = 2.f * jobs[k].th;
            S.searches = 2;
            results[k].searches = 2;
            again = true;
        }
    }
    if (!again) idle_call(C, ORBGPU_PROJ_LAST_FRAME);
}

__global__ __launch_bounds__(kThreads) void initial_gather_kernel(const orbgpu_track_initial_job* __restrict__ jobs,
                                                                  const orbgpu_reloc_frame* __restrict__ frames,
                                                                  int stride, IWork V,
                                                                  orbgpu_track_initial_result* __restrict__ results,
                                                                  int* __restrict__ rows) {
    __shared__ int s_wave[kThreads / 64];
    __shared__ float s_T[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    IFrame& S = V.st[k];
    if (S.status != kPending) return;  // its job is already empty
    const orbgpu_track_initial_job& J = jobs[k];
    orbgpu_track_initial_result& R = results[k];
    const bool motion = J.mode == ORBGPU_TRACK_MOTION;
    const size_t o = (size_t)k * stride;
    const int searches = S.searches, nf = S.nf, np = S.np;
    const int* row;
    int nm;
    if (motion) {
        row = V.pm[searches - 1] + o;
        nm = searches == 2 ? V.pn[1][k] : S.n1;
    } else {
        row = J.bow_row;
        nm = *J.bow_nmatches;
    }
    if (tid < 16) s_T[tid] = J.Tcw_init[tid];
    __syncthreads();  // every lane has read S before lane 0 writes it
    const bool few = nm < (motion ? ORBGPU_TRACK_MIN_MATCHES : ORBGPU_TRACK_MIN_BOW_MATCHES);
    if (tid == 0) {
        if (motion && searches == 2) R.nsearch[1] = nm;
        R.nmatches = nm;
        S.nm = nm;
        if (few) {  // `return false` before the optimisation (:992, :1162): the pose stays the start
            S.status = R.status = (motion && nm < 0) ? ORBGPU_TRACK_CAPACITY : ORBGPU_TRACK_FEW_MATCHES;
            for (int i = 0; i < 16; ++i) R.Tcw[i] = s_T[i];
        }
    }
    if (few) return;
    // only entries >= 0 become mvpMapPoints: a -2 was this call's own assignment on a NULL row
    int* mp = V.mp + o;
    int* rw = rows + (size_t)k * ORBGPU_TRACK_INITIAL_ROWS * stride;
    for (int j = tid; j < nf; j += kThreads) {
        int p = row[j];
        if (p < 0 || p >= np) p = -1;
        mp[j] = p;
        rw[j] = p;
    }
    __syncthreads();
    const Gather G{V.jobs + k, V.Xw + 3 * o, V.obs + 3 * o, V.w + o, V.gidx + o};
    gather_job(frames[J.frame], nf, mp, J.points.pos, s_T, k * stride, G, s_wave);
}

__global__ __launch_bounds__(kThreads) void initial_cull_kernel(const orbgpu_track_initial_job* __restrict__ jobs,
                                                                int stride, IWork V,
                                                                orbgpu_track_initial_result* __restrict__ results,
                                                                int* __restrict__ rows) {
    __shared__ int s_out, s_map;
    const int k = blockIdx.x, tid = threadIdx.x;
    IFrame& S = V.st[k];
    if (S.status != kPending) return;
    const orbgpu_track_initial_job& J = jobs[k];
    orbgpu_track_initial_result& R = results[k];
    const size_t o = (size_t)k * stride;
    int* mp = V.mp + o;
    int* rw = rows + (size_t)k * ORBGPU_TRACK_INITIAL_ROWS * stride + stride;
    const int n = min(max(V.jobs[k].n, 0), stride), nf = S.nf;
    if (tid == 0) s_out = s_map = 0;
    __syncthreads();
    int n_out = 0, n_map = 0;
    for (int i = tid; i < n; i += kThreads) {  // :1172-1189
        const int j = V.gidx[o + i];
        if (V.outl[o + i]) {
            mp[j] = -1;
            ++n_out;
        } else if (J.points.flags[mp[j]] & ORBGPU_PT_HAS_OBS) {
            ++n_map;
        }
    }
    if (n_out) atomicAdd(&s_out, n_out);
    if (n_map) atomicAdd(&s_map, n_map);
    __syncthreads();
    for (int j = tid; j < nf; j += kThreads) rw[j] = mp[j];
    if (tid == 0) {
        const int nmatches = S.nm - s_out, nmap = s_map;
        bool ok = nmap >= ORBGPU_TRACK_MIN_MAP_MATCHES;
        R.vo = 0;
        if (J.mode == ORBGPU_TRACK_MOTION && J.only_tracking) {  // :1191-1195
            R.vo = nmap < ORBGPU_TRACK_MIN_MAP_MATCHES;
            ok = nmatches > ORBGPU_TRACK_MIN_MATCHES;
        }
        R.nmatches = nmatches;
        R.nmatches_map = nmap;
        copy_opt(R.opt, V.opt[k]);
        for (int i = 0; i < 16; ++i) R.Tcw[i] = V.opt[k].Tcw[i];
        S.status = R.status = ok ? ORBGPU_TRACK_OK : ORBGPU_TRACK_LOST;
    }
}

// ------------------------------------------------------------------ 2. the local map

// proj.hip's float helpers, restated (Frame.cpp:305-368, MapPoint.cpp:481-508)
__device__ inline float dotd3(const float* a, const float* x) {  // cv::Mat float product, double accumulation
    return (float)((double)a[0] * (double)x[0] + (double)a[1] * (double)x[1] + (double)a[2] * (double)x[2]);
}
__device__ inline void transform(const float* T, const float* x, float* y) {
    for (int i = 0; i < 3; ++i) {
        const float r[3] = {T[4 * i], T[4 * i + 1], T[4 * i + 2]};
        y[i] = dotd3(r, x) + T[4 * i + 3];
    }
}
__device__ inline void camera_center(const float* T, float* O) {
    for (int j = 0; j < 3; ++j) {
        const float c[3] = {T[j], T[4 + j], T[8 + j]};
        const float t[3] = {T[3], T[7], T[11]};
        O[j] = -dotd3(c, t);
    }
}
__device__ inline int predict_scale(float max_dist, float dist, float log_scale_factor, int n_levels) {
    const float ratio = max_dist / dist;
    const float l = (float)log((double)ratio);
    int s = (int)ceilf(l / log_scale_factor);
    if (s < 0) s = 0;
    else if (s >= n_levels) s = n_levels - 1;
    return s;
}

struct LFrame {
    int status;
    int nf, np, n_local;
    int n_to_match;
    int pad[3];
    float Tcw[16];  // the pose as read from HBM when the call ran
};

struct LWork {
    LFrame* st;
    int* mp;
    uint8_t* occ;
    int* wflags;   // the call's point flags: the table's with ORBGPU_PT_IN_VIEW
    float* track;  // 4 per point
    int* level;
    int* pm;
    int* pn;
    orbgpu_proj_call* calls;
    orbgpu_poseopt_job* jobs;
    orbgpu_poseopt_result* opt;
    float *Xw, *obs, *w;
    int* gidx;
    uint8_t* outl;
};

inline LWork carve_local(void* base, int n, int stride, int point_stride, size_t* bytes) {
    const size_t N = (size_t)(n > 0 ? n : 1), S = (size_t)(stride > 0 ? stride : 1),
                 P = (size_t)(point_stride > 0 ? point_stride : 1);
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    LWork v;
    v.st = take<LFrame>(p, N);
    v.mp = take<int>(p, N * S);
    v.occ = take<uint8_t>(p, N * S);
    v.wflags = take<int>(p, N * P);
    v.track = take<float>(p, 4 * N * P);
    v.level = take<int>(p, N * P);
    v.pm = take<int>(p, N * S);
    v.pn = take<int>(p, N);
    v.calls = take<orbgpu_proj_call>(p, N);
    v.jobs = take<orbgpu_poseopt_job>(p, N);
    v.opt = take<orbgpu_poseopt_result>(p, N);
    v.Xw = take<float>(p, 3 * N * S);
    v.obs = take<float>(p, 3 * N * S);
    v.w = take<float>(p, N * S);
    v.gidx = take<int>(p, N * S);
    v.outl = take<uint8_t>(p, N * S);
    if (bytes) *bytes = (size_t)(p - reinterpret_cast<uintptr_t>(base));
    return v;
}

__global__ __launch_bounds__(kThreads) void local_begin_kernel(const orbgpu_track_local_job* __restrict__ jobs,
                                                               int n_frames,
                                                               const orbgpu_reloc_frame* __restrict__ frames, int stride,
                                                               int point_stride, LWork V,
                                                               orbgpu_track_local_result* __restrict__ results,
                                                               int* __restrict__ rows, uint8_t* __restrict__ point_flags) {
    __shared__ int s_status, s_count;
    __shared__ float s_T[16], s_O[3];
    const int k = blockIdx.x, tid = threadIdx.x;
    const orbgpu_track_local_job& J = jobs[k];
    const size_t o = (size_t)k * stride, op = (size_t)k * point_stride;
    int* rw = rows + (size_t)k * ORBGPU_TRACK_LOCAL_ROWS * stride;
    uint8_t* pf = point_flags + op;
    for (int i = tid; i < stride; i += kThreads) {
        rw[i] = rw[stride + i] = -1;
        rw[2 * (size_t)stride + i] = 0;  // mvbOutlier is false wherever call 1 left a point, and elsewhere
        V.mp[o + i] = -1;
        V.occ[o + i] = 0;
    }
    for (int i = tid; i < point_stride; i += kThreads) pf[i] = 0;
    if (tid == 0) {
        orbgpu_track_local_result& R = results[k];
        zero_words(&R, sizeof(R));
        R.nsearch = -1;
        LFrame& S = V.st[k];
        zero_words(&S, sizeof(S));
        idle_call(V.calls[k], ORBGPU_PROJ_LOCAL);
        empty_job(V.jobs[k], k * stride);
        int status = kPending;
        if (J.frame < 0 || J.frame >= n_frames || J.points.n < 0 || J.n_local < 0 || J.n_local > J.points.n || !J.Tcw ||
            !J.frame_mp) {
            status = ORBGPU_TRACK_BAD_JOB;
        } else {
            const int nf = frames[J.frame].target.n;
            if (nf < 0 || nf > min(stride, kMaxKps) || J.points.n > point_stride) {
                status = ORBGPU_TRACK_CAPACITY;
            } else {
                S.nf = nf;
                S.np = J.points.n;
                S.n_local = J.n_local;
            }
        }
        S.status = status;
        R.status = status == kPending ? ORBGPU_TRACK_OK : status;
        s_status = status;
        s_count = 0;
    }
    __syncthreads();
    if (s_status != kPending) return;
    LFrame& S = V.st[k];
    const orbgpu_reloc_frame& F = frames[J.frame];
    const orbgpu_proj_target& T = F.target;
    const int nf = S.nf, np = S.np, n_local = S.n_local;
    if (tid < 16) s_T[tid] = S.Tcw[tid] = J.Tcw[tid];
    __syncthreads();
    if (tid == 0) camera_center(s_T, s_O);
    // :1501-1520: a held bad point is nulled, every other held point is seen
    int* mp = V.mp + o;
    for (int j = tid; j < nf; j += kThreads) {
        int p = J.frame_mp[j];
        if (p < 0 || p >= np || !(J.points.flags[p] & ORBGPU_PT_VALID)) p = -1;
        mp[j] = p;
        if (p >= 0) pf[p] = ORBGPU_TRACK_PT_SEEN;
    }
    __syncthreads();
    // :1526-1545: isInFrustum(pMP, 0.5) of every good local point not seen (Frame.cpp:305-368)
    int count = 0;
    for (int i = tid; i < n_local; i += kThreads) {
        const int fl = J.points.flags[i];
        int wf = fl & (ORBGPU_PT_VALID | ORBGPU_PT_HAS_OBS);  // mbTrackInView = false
        // mnLastFrameSeen == mnId (:1531): held by the frame, or culled by call 1 (:1016, :1183)
        if ((fl & ORBGPU_PT_VALID) && !(fl & ORBGPU_PT_LAST_SEEN) && !(pf[i] & ORBGPU_TRACK_PT_SEEN)) {
            const float X[3] = {J.points.pos[3 * (size_t)i], J.points.pos[3 * (size_t)i + 1], J.points.pos[3 * (size_t)i + 2]};
            float pc[3];
            transform(s_T, X, pc);
            bool ok = !(pc[2] < 0.0f);
            float u = 0.f, v = 0.f, invz = 0.f, viewCos = 0.f, dist = 0.f;
            if (ok) {
                invz = 1.0f / pc[2];
                u = T.fx * pc[0] * invz + T.cx;
                v = T.fy * pc[1] * invz + T.cy;
                if (u < T.min_x || u > T.max_x || v < T.min_y || v > T.max_y) ok = false;
            }
            if (ok) {
                const float maxd = 1.2f * J.points.max_dist[i], mind = 0.8f * J.points.min_dist[i];
                const float PO[3] = {X[0] - s_O[0], X[1] - s_O[1], X[2] - s_O[2]};
                dist = (float)sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
                if (dist < mind || dist > maxd) ok = false;
                else {
                    const float* Pn = J.points.normal + 3 * (size_t)i;
                    viewCos = (float)(((double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2]) / dist);
                    if (viewCos < 0.5f) ok = false;
                }
            }
            if (ok) {
                wf |= ORBGPU_PT_IN_VIEW;
                float* tr = V.track + 4 * (op + i);
                tr[0] = u;
                tr[1] = v;
                tr[2] = u - T.bf * invz;
                tr[3] = viewCos;
                V.level[op + i] = predict_scale(J.points.max_dist[i], dist, T.log_scale_factor, T.n_levels);
                pf[i] = ORBGPU_TRACK_PT_IN_VIEW;
                ++count;
            }
        }
        V.wflags[op + i] = wf;
    }
    if (count) atomicAdd(&s_count, count);
    // the occupancy the search sees: 0 NULL, 1 a point without observations, 2 one with (ORBmatcher.cpp:113)
    for (int j = tid; j < nf; j += kThreads) {
        const int p = mp[j];
        V.occ[o + j] = p < 0 ? 0 : ((J.points.flags[p] & ORBGPU_PT_HAS_OBS) ? 2 : 1);
    }
    __syncthreads();
    if (tid == 0) {
        const int n_to_match = s_count;
        S.n_to_match = n_to_match;
        results[k].n_to_match = n_to_match;
        if (n_to_match > 0) {  // ORBmatcher matcher(0.8); matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th)
            orbgpu_proj_call& C = V.calls[k];
            C.nnratio = 0.8f;
            C.th = J.th;
            C.target = T;
            C.target.occupied = V.occ + o;
            for (int i = 0; i < 16; ++i) C.target.Tcw[i] = s_T[i];
            C.points = J.points;
            C.points.n = n_local;
            C.points.flags = V.wflags + op;
            C.points.track = V.track + 4 * op;
            C.points.track_level = V.level + op;
        }
    }
}

__global__ __launch_bounds__(kThreads) void local_gather_kernel(const orbgpu_track_local_job* __restrict__ jobs,
                                                                const orbgpu_reloc_frame* __restrict__ frames,
                                                                int stride, LWork V,
                                                                orbgpu_track_local_result* __restrict__ results,
                                                                int* __restrict__ rows) {
    __shared__ int s_wave[kThreads / 64];
    __shared__ float s_T[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    LFrame& S = V.st[k];
    if (S.status != kPending) return;
    const orbgpu_track_local_job& J = jobs[k];
    const size_t o = (size_t)k * stride;
    const int nf = S.nf, n_local = S.n_local;
    const bool searched = S.n_to_match > 0;
    const int ns = searched ? V.pn[k] : -1;
    if (tid < 16) s_T[tid] = S.Tcw[tid];
    __syncthreads();
    if (searched && ns < 0) {  // over the matcher's capacity after all: the frame ends, nothing truncated
        if (tid == 0) S.status = results[k].status = ORBGPU_TRACK_CAPACITY;
        return;
    }
    if (tid == 0) results[k].nsearch = ns;
    int* mp = V.mp + o;
    int* rw = rows + (size_t)k * ORBGPU_TRACK_LOCAL_ROWS * stride;
    for (int j = tid; j < nf; j += kThreads) {
        if (searched) {
            const int p = V.pm[o + j];
            if (p >= 0 && p < n_local) mp[j] = p;
        }
        rw[j] = mp[j];
    }
    __syncthreads();
    const Gather G{V.jobs + k, V.Xw + 3 * o, V.obs + 3 * o, V.w + o, V.gidx + o};
    gather_job(frames[J.frame], nf, mp, J.points.pos, s_T, k * stride, G, s_wave);
}

__global__ __launch_bounds__(kThreads) void local_decide_kernel(const orbgpu_track_local_job* __restrict__ jobs,
                                                                int stride, LWork V,
                                                                orbgpu_track_local_result* __restrict__ results,
                                                                int* __restrict__ rows) {
    __shared__ int s_inl;
    const int k = blockIdx.x, tid = threadIdx.x;
    LFrame& S = V.st[k];
    if (S.status != kPending) return;
    const orbgpu_track_local_job& J = jobs[k];
    orbgpu_track_local_result& R = results[k];
    const size_t o = (size_t)k * stride;
    int* mp = V.mp + o;
    int* rw = rows + (size_t)k * ORBGPU_TRACK_LOCAL_ROWS * stride;
    const int n = min(max(V.jobs[k].n, 0), stride), nf = S.nf;
    if (tid == 0) s_inl = 0;
    __syncthreads();
    int inl = 0;
    for (int i = tid; i < n; i += kThreads) {  // :1230-1252
        const int j = V.gidx[o + i];
        if (!V.outl[o + i]) {
            if (J.only_tracking || (J.points.flags[mp[j]] & ORBGPU_PT_HAS_OBS)) ++inl;
        } else {
            rw[2 * (size_t)stride + j] = 1;
            if (J.stereo) mp[j] = -1;
        }
    }
    if (inl) atomicAdd(&s_inl, inl);
    __syncthreads();
    for (int j = tid; j < nf; j += kThreads) rw[stride + j] = mp[j];
    if (tid == 0) {
        const int n_inl = s_inl;
        R.n_inliers = n_inl;
        copy_opt(R.opt, V.opt[k]);
        for (int i = 0; i < 16; ++i) R.Tcw[i] = V.opt[k].Tcw[i];
        const bool lost = (J.recently_relocalised && n_inl < 50) || n_inl < 30;  // :1257-1263
        S.status = R.status = lost ? ORBGPU_TRACK_LOST : ORBGPU_TRACK_OK;
    }
}

// ------------------------------------------------------------------ 3. UpdateLastFrame

__global__ __launch_bounds__(kThreads) void update_last_frame_kernel(const orbgpu_update_last_frame_job* __restrict__ jobs,
                                                                     int stride,
                                                                     orbgpu_update_last_frame_result* __restrict__ results,
                                                                     uint8_t* __restrict__ created) {
    __shared__ float s_z[kMaxKps];  // the depth of a slot with z > 0, else 0
    __shared__ int s_pos, s_close, s_created;
    const int k = blockIdx.x, tid = threadIdx.x;
    const orbgpu_update_last_frame_job& J = jobs[k];
    uint8_t* cr = created + (size_t)k * stride;
    for (int i = tid; i < stride; i += kThreads) cr[i] = 0;
    const int n = J.n;
    if (n < 0 || n > min(stride, kMaxKps)) {
        if (tid == 0) {
            orbgpu_update_last_frame_result& R = results[k];
            R.status = ORBGPU_TRACK_CAPACITY;
            R.n_created = R.n_pos = R.n_visited = 0;
        }
        return;
    }
    if (tid == 0) s_pos = s_close = s_created = 0;
    __syncthreads();
    const float th = J.th_depth;
    int n_pos = 0, n_close = 0;
    for (int i = tid; i < n; i += kThreads) {
        const float z = J.depth[i];
        const bool pos = z > 0;  // :1059; false for NaN
        s_z[i] = pos ? z : 0.f;
        n_pos += pos;
        n_close += pos && !(z > th);  // the loop's `>` (:1111), so a NaN th_depth never ends it
    }
    if (n_pos) atomicAdd(&s_pos, n_pos);
    if (n_close) atomicAdd(&s_close, n_close);
    __syncthreads();
    // both branches count (:1104, :1108): the loop ends after visiting index max(m, 100) of the order
    const int n_vis = min(s_pos, max(s_close, 100) + 1);
    int n_new = 0;
    for (int i = tid; i < n; i += kThreads) {
        const float z = s_z[i];
        if (!(z > 0)) continue;
        int rank = 0;  // the slots before (z, i) in std::sort's order of pair<float, int>
        for (int a = 0; a < n; ++a) {
            const float za = s_z[a];
            rank += za > 0 && (za < z || (za == z && a < i));
        }
        if (rank >= n_vis) continue;
        const int fl = J.flags[i];
        if ((fl & ORBGPU_PT_VALID) && (fl & ORBGPU_PT_HAS_OBS)) continue;  // pMP with Observations() >= 1 (:1081-1087)
        // Frame::UnprojectStereo (Frame.cpp:787-795): mRwc * x3Dc accumulates in double, + mOw in float
        const orbgpu_keypoint kp = J.kps_un[i];
        const float x = (kp.x - J.cx) * z * J.invfx;
        const float y = (kp.y - J.cy) * z * J.invfy;
        for (int r = 0; r < 3; ++r) {
            const float m = (float)((double)J.Rwc[3 * r] * x + (double)J.Rwc[3 * r + 1] * y + (double)J.Rwc[3 * r + 2] * z);
            J.pos[3 * (size_t)i + r] = m + J.Ow[r];
        }
        const uint4* src = reinterpret_cast<const uint4*>(J.frame_desc + 32 * (size_t)i);
        uint4* dst = reinterpret_cast<uint4*>(J.desc + 32 * (size_t)i);
        dst[0] = src[0];
        dst[1] = src[1];
        J.flags[i] = (fl | ORBGPU_PT_VALID) & ~ORBGPU_PT_HAS_OBS;
        cr[i] = 1;
        ++n_new;
    }
    if (n_new) atomicAdd(&s_created, n_new);
    __syncthreads();
    if (tid == 0) {
        orbgpu_update_last_frame_result& R = results[k];
        R.status = ORBGPU_TRACK_OK;
        R.n_created = s_created;
        R.n_pos = s_pos;
        R.n_visited = n_vis;
    }
}

bool fits_int(long long a, long long b) { return a * b <= 0x7fffffffLL; }

}  // namespace

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

size_t orbgpu_track_initial_workspace_bytes(int n, int stride) {
    if (!fits_int(n > 0 ? n : 1, 3LL * (stride > 0 ? stride : 1))) return 0;
    size_t bytes = 0;
    carve_initial(nullptr, n, stride, &bytes);
    return bytes;
}

int orbgpu_track_initial_batch_device(int n, const orbgpu_track_initial_job* d_jobs, int n_frames,
                                      const orbgpu_reloc_frame* d_frames, int stride, void* d_workspace,
                                      orbgpu_track_initial_result* d_results, int* d_rows, void* stream) {
    if (n < 0 || n_frames < 0 || stride <= 0 || (n > 0 && (!d_jobs || !d_frames || !d_workspace || !d_results || !d_rows)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if (!fits_int(n, 3LL * stride)) return fail(ORBGPU_ERR_ARG, "n * stride overflows");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const IWork V = carve_initial(d_workspace, n, stride, nullptr);
    const dim3 grid(n), block(kThreads);
    hipLaunchKernelGGL(initial_begin_kernel, grid, block, 0, s, d_jobs, n_frames, d_frames, stride, V, d_results, d_rows);
    ORB_HIP(hipGetLastError());
    if (int rc = orbgpu_search_by_projection_batch_device(n, V.calls, stride, V.pm[0], V.pn[0], stream)) return rc;
    hipLaunchKernelGGL(initial_retry_kernel, grid, dim3(64), 0, s, d_jobs, V, d_results);
    ORB_HIP(hipGetLastError());
    if (int rc = orbgpu_search_by_projection_batch_device(n, V.calls, stride, V.pm[1], V.pn[1], stream)) return rc;
    hipLaunchKernelGGL(initial_gather_kernel, grid, block, 0, s, d_jobs, d_frames, stride, V, d_results, d_rows);
    ORB_HIP(hipGetLastError());
    if (int rc = orbgpu_pose_optimization_batch_device(n, V.jobs, n * stride, V.Xw, V.obs, V.w, V.opt, V.outl, stream))
        return rc;
    hipLaunchKernelGGL(initial_cull_kernel, grid, block, 0, s, d_jobs, stride, V, d_results, d_rows);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

size_t orbgpu_track_local_workspace_bytes(int n, int stride, int point_stride) {
    const long long N = n > 0 ? n : 1;
    if (!fits_int(N, 3LL * (stride > 0 ? stride : 1)) || !fits_int(N, 4LL * (point_stride > 0 ? point_stride : 1))) return 0;
    size_t bytes = 0;
    carve_local(nullptr, n, stride, point_stride, &bytes);
    return bytes;
}

int orbgpu_track_local_map_batch_device(int n, const orbgpu_track_local_job* d_jobs, int n_frames,
                                        const orbgpu_reloc_frame* d_frames, int stride, int point_stride,
                                        void* d_workspace, orbgpu_track_local_result* d_results, int* d_rows,
                                        uint8_t* d_point_flags, void* stream) {
    if (n < 0 || n_frames < 0 || stride <= 0 || point_stride <= 0 ||
        (n > 0 && (!d_jobs || !d_frames || !d_workspace || !d_results || !d_rows || !d_point_flags)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if (!fits_int(n, 3LL * stride) || !fits_int(n, 4LL * point_stride))
        return fail(ORBGPU_ERR_ARG, "n * stride or n * point_stride overflows");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const LWork V = carve_local(d_workspace, n, stride, point_stride, nullptr);
    const dim3 grid(n), block(kThreads);
    hipLaunchKernelGGL(local_begin_kernel, grid, block, 0, s, d_jobs, n_frames, d_frames, stride, point_stride, V,
                       d_results, d_rows, d_point_flags);
    ORB_HIP(hipGetLastError());
    if (int rc = orbgpu_search_by_projection_batch_device(n, V.calls, stride, V.pm, V.pn, stream)) return rc;
    hipLaunchKernelGGL(local_gather_kernel, grid, block, 0, s, d_jobs, d_frames, stride, V, d_results, d_rows);
    ORB_HIP(hipGetLastError());
    if (int rc = orbgpu_pose_optimization_batch_device(n, V.jobs, n * stride, V.Xw, V.obs, V.w, V.opt, V.outl, stream))
        return rc;
    hipLaunchKernelGGL(local_decide_kernel, grid, block, 0, s, d_jobs, stride, V, d_results, d_rows);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

int orbgpu_update_last_frame_batch_device(int n, const orbgpu_update_last_frame_job* d_jobs, int stride,
                                          orbgpu_update_last_frame_result* d_results, uint8_t* d_created,
                                          void* stream) {
    if (n < 0 || stride <= 0 || (n > 0 && (!d_jobs || !d_results || !d_created)))
        return fail(ORBGPU_ERR_ARG, "invalid argument");
    if (!fits_int(n, stride)) return fail(ORBGPU_ERR_ARG, "n * stride overflows");
    if (n == 0) return ORBGPU_OK;
    if (int rc = check_device()) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(update_last_frame_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, d_jobs, stride,
                       d_results, d_created);
    ORB_HIP(hipGetLastError());
    return ORBGPU_OK;
}

}  // extern "C"
