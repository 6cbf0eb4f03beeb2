// covis_update_args_main.cpp -- the host side of csrc/covis.hip's UpdateConnections and KeyFrameCulling on its own,
// for tests/test_covis_update.py, in the manner of covis_args_main.cpp: the calls with VALID arguments (which a
// Python test must not make, since on a machine with a device they are launches) and the argument checks,
// compiled for the host under the address and undefined-behaviour sanitizers.  No HIP runtime is linked: the few
// names the host code refers to are defined here, and the device check answers that there is no device, so
// nothing is launched.  Every pointer is a real allocation of the size its call would read or write.
//   covis_update_args_main          runs the checks, prints "ok"
//   covis_update_args_main sizes    prints the sizes and offsets of the new structs
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../orb-slam2-annotation_amd/csrc/covis.hip"

// ---- what liborbgpu.so and the HIP runtime would provide
namespace orbgpu {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int check_device() { return fail(ORBGPU_ERR_NO_DEVICE, "no device"); }
}  // namespace orbgpu

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "no HIP runtime"; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { return nullptr; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

#define EXPECT(cond)                                                                        \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "covis_update_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static int sizes() {
    std::printf("orbgpu_covis_update_result %zu\n", sizeof(orbgpu_covis_update_result));
    std::printf("update_result.n_counted %zu\n", offsetof(orbgpu_covis_update_result, n_counted));
    std::printf("update_result.n_ordered %zu\n", offsetof(orbgpu_covis_update_result, n_ordered));
    std::printf("update_result.kf_max %zu\n", offsetof(orbgpu_covis_update_result, kf_max));
    std::printf("update_result.w_max %zu\n", offsetof(orbgpu_covis_update_result, w_max));
    std::printf("update_result.front %zu\n", offsetof(orbgpu_covis_update_result, front));
    std::printf("orbgpu_map_mirror_cull %zu\n", sizeof(orbgpu_map_mirror_cull));
    std::printf("mirror_cull.kp_depth %zu\n", offsetof(orbgpu_map_mirror_cull, kp_depth));
    std::printf("mirror_cull.kf_th_depth %zu\n", offsetof(orbgpu_map_mirror_cull, kf_th_depth));
    std::printf("mirror_cull.kf_not_erase %zu\n", offsetof(orbgpu_map_mirror_cull, kf_not_erase));
    std::printf("orbgpu_covis_cull_job %zu\n", sizeof(orbgpu_covis_cull_job));
    std::printf("cull_job.mono %zu\n", offsetof(orbgpu_covis_cull_job, mono));
    std::printf("orbgpu_covis_cull_verdict %zu\n", sizeof(orbgpu_covis_cull_verdict));
    std::printf("cull_verdict.n_mps %zu\n", offsetof(orbgpu_covis_cull_verdict, n_mps));
    std::printf("cull_verdict.n_redundant %zu\n", offsetof(orbgpu_covis_cull_verdict, n_redundant));
    std::printf("cull_verdict.verdict %zu\n", offsetof(orbgpu_covis_cull_verdict, verdict));
    std::printf("orbgpu_covis_cull_result %zu\n", sizeof(orbgpu_covis_cull_result));
    std::printf("cull_result.n_list %zu\n", offsetof(orbgpu_covis_cull_result, n_list));
    std::printf("cull_result.n_culled %zu\n", offsetof(orbgpu_covis_cull_result, n_culled));
    std::printf("cull_result.n_to_be_erased %zu\n", offsetof(orbgpu_covis_cull_result, n_to_be_erased));
    std::printf("status.EMPTY %d\n", (int)ORBGPU_COVIS_EMPTY);
    std::printf("status.CAPACITY %d\n", (int)ORBGPU_COVIS_CAPACITY);
    std::printf("verdict.KEPT %d\n", (int)ORBGPU_COVIS_CULL_KEPT);
    std::printf("verdict.CULLED %d\n", (int)ORBGPU_COVIS_CULL_CULLED);
    std::printf("verdict.TO_BE_ERASED %d\n", (int)ORBGPU_COVIS_CULL_TO_BE_ERASED);
    std::printf("verdict.SKIPPED_FIRST %d\n", (int)ORBGPU_COVIS_CULL_SKIPPED_FIRST);
    std::printf("th %d\n", (int)ORBGPU_COVIS_TH);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    static_assert(ORBGPU_COVIS_CAPACITY == ORBGPU_LOCALMAP_CAPACITY && ORBGPU_COVIS_BAD_JOB == ORBGPU_LOCALMAP_BAD_JOB, "");
    // a map of 4 keyframes with 3 slots each, 5 points with 2 observations each, and its table: real arrays of
    // the right sizes, though nothing reads them here
    const int n_kf = 4, n_pt = 5, stride = 8, n = 2, list_stride = 8;
    std::vector<int> slot_offset{0, 3, 6, 9}, n_slots(n_kf, 3), slots(12, -1), by_rank{3, 2, 1, 0};
    std::vector<int> pt_flags(n_pt, 1), obs_offset{0, 2, 4, 6, 8}, n_obs(n_pt, 2), obs(10, 0), obs_idx(10, 0);
    std::vector<uint8_t> kf_first(n_kf, 0), kf_not_erase(n_kf, 0), kp_octave(12, 0);
    std::vector<float> kp_obs(36, 0.f), kp_depth(12, 1.f), kf_th_depth(n_kf, 35.f);
    std::vector<int> n_conn(n_kf, 0), n_ord(n_kf, 0), rows(4 * n_kf * stride, 0), covis10(n_kf * ORBGPU_COVIS_BEST, -1);
    orbgpu_map_mirror mirror;
    std::memset(&mirror, 0, sizeof(mirror));
    mirror.n_kf = n_kf, mirror.n_pt = n_pt, mirror.n_slots_total = 12, mirror.n_obs_total = 10;
    mirror.slot_offset = slot_offset.data(), mirror.n_slots = n_slots.data(), mirror.slots = slots.data();
    mirror.kf_by_rank = by_rank.data(), mirror.pt_flags = pt_flags.data(), mirror.obs_offset = obs_offset.data();
    mirror.n_obs = n_obs.data(), mirror.obs = obs.data();
    orbgpu_map_mirror_ba ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.kf_first = kf_first.data(), ba.kp_obs = kp_obs.data(), ba.obs_idx = obs_idx.data();
    orbgpu_map_mirror_cull cull{kp_octave.data(), kp_depth.data(), kf_th_depth.data(), kf_not_erase.data()};
    orbgpu_covis_graph graph;
    graph.n_kf = n_kf, graph.conn_stride = stride, graph.n_conn = n_conn.data(), graph.n_ord = n_ord.data();
    graph.conn_kf = rows.data(), graph.conn_w = rows.data() + n_kf * stride, graph.ord_kf = rows.data() + 2 * n_kf * stride;
    graph.ord_w = rows.data() + 3 * n_kf * stride, graph.covis10 = covis10.data();
    std::vector<int> kfs{1, 2};
    std::vector<orbgpu_covis_update_result> ures(n);
    const size_t ws_bytes = orbgpu_covis_update_workspace_bytes(n, n_kf);
    EXPECT(ws_bytes == sizeof(int) * (n_kf + 1 + n + n * n_kf));
    EXPECT(orbgpu_covis_update_workspace_bytes(-1, 4) == 0 && orbgpu_covis_update_workspace_bytes(4, -1) == 0);
    EXPECT(orbgpu_covis_update_workspace_bytes(1 << 16, 1 << 16) == 0);
    EXPECT(orbgpu_covis_update_workspace_bytes(0, 0) == sizeof(int));
    std::vector<char> ws(ws_bytes);

    auto update = [&](int nn, const int* k, const orbgpu_map_mirror* m, const orbgpu_covis_graph* g, void* w, size_t wb,
                      orbgpu_covis_update_result* r) {
        return orbgpu_covis_update_connections_batch_device(nn, k, m, g, w, wb, r, nullptr);
    };
    // valid: the device check
    EXPECT(update(n, kfs.data(), &mirror, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_NO_DEVICE);
    {
        orbgpu_map_mirror m = mirror;
        m.kf_by_rank = nullptr;  // ascending index
        EXPECT(update(n, kfs.data(), &m, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_NO_DEVICE);
    }
    EXPECT(update(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == ORBGPU_OK);  // nothing to do
    EXPECT(update(0, nullptr, &mirror, &graph, nullptr, 0, nullptr) == ORBGPU_OK);
    EXPECT(update(-1, kfs.data(), &mirror, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
    EXPECT(update(n, nullptr, &mirror, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
    EXPECT(update(n, kfs.data(), nullptr, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
    EXPECT(update(n, kfs.data(), &mirror, nullptr, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
    EXPECT(update(n, kfs.data(), &mirror, &graph, nullptr, ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
    EXPECT(update(n, kfs.data(), &mirror, &graph, ws.data(), ws_bytes - 1, ures.data()) == ORBGPU_ERR_ARG);  // short
    EXPECT(update(n, kfs.data(), &mirror, &graph, ws.data(), ws_bytes, nullptr) == ORBGPU_ERR_ARG);
    {
        orbgpu_covis_graph g = graph;
        g.n_kf = n_kf - 1;  // not the mirror's
        EXPECT(update(n, kfs.data(), &mirror, &g, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
        g = graph;
        g.conn_stride = 0;
        EXPECT(update(n, kfs.data(), &mirror, &g, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
        g = graph;
        g.ord_w = nullptr;
        EXPECT(update(n, kfs.data(), &mirror, &g, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
        EXPECT(update(0, nullptr, &mirror, &g, nullptr, 0, nullptr) == ORBGPU_ERR_ARG);  // a graph given is checked
    }
    const size_t read_arrays[] = {offsetof(orbgpu_map_mirror, slot_offset), offsetof(orbgpu_map_mirror, n_slots),
                                  offsetof(orbgpu_map_mirror, slots),       offsetof(orbgpu_map_mirror, pt_flags),
                                  offsetof(orbgpu_map_mirror, obs_offset),  offsetof(orbgpu_map_mirror, n_obs),
                                  offsetof(orbgpu_map_mirror, obs)};
    std::vector<orbgpu_covis_cull_job> jobs{{1, 0}, {2, 1}};
    std::vector<orbgpu_covis_cull_result> cres(n);
    std::vector<orbgpu_covis_cull_verdict> verdicts(n * list_stride);
    std::vector<int> culled(n * list_stride);
    auto cullf = [&](int nn, const orbgpu_covis_cull_job* j, const orbgpu_map_mirror* m, const orbgpu_map_mirror_ba* b,
                     const orbgpu_map_mirror_cull* c, const orbgpu_covis_graph* g, int ls, orbgpu_covis_cull_result* r,
                     orbgpu_covis_cull_verdict* v, int* cu) {
        return orbgpu_covis_keyframe_culling_batch_device(nn, j, m, b, c, g, ls, r, v, cu, nullptr);
    };
    for (size_t off : read_arrays) {
        orbgpu_map_mirror m = mirror;
        std::memset(reinterpret_cast<char*>(&m) + off, 0, sizeof(void*));
        EXPECT(update(n, kfs.data(), &m, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
        EXPECT(cullf(n, jobs.data(), &m, &ba, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) ==
               ORBGPU_ERR_ARG);
    }
    for (int which = 0; which < 4; ++which) {
        orbgpu_map_mirror m = mirror;
        (which == 0 ? m.n_kf : which == 1 ? m.n_pt : which == 2 ? m.n_slots_total : m.n_obs_total) = -1;
        EXPECT(update(n, kfs.data(), &m, &graph, ws.data(), ws_bytes, ures.data()) == ORBGPU_ERR_ARG);
    }

    // ---- KeyFrameCulling
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) ==
           ORBGPU_ERR_NO_DEVICE);  // valid: the device check
    EXPECT(cullf(0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr) == ORBGPU_OK);
    EXPECT(cullf(0, nullptr, &mirror, &ba, &cull, &graph, list_stride, nullptr, nullptr, nullptr) == ORBGPU_OK);
    EXPECT(cullf(-1, jobs.data(), &mirror, &ba, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) ==
           ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &graph, 0, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &graph, 0x7fffffff, cres.data(), verdicts.data(), culled.data()) ==
           ORBGPU_ERR_ARG);  // n * list_stride
    EXPECT(cullf(n, nullptr, &mirror, &ba, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), nullptr, &ba, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, nullptr, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, nullptr, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, nullptr, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &graph, list_stride, nullptr, verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &graph, list_stride, cres.data(), nullptr, culled.data()) == ORBGPU_ERR_ARG);
    EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &graph, list_stride, cres.data(), verdicts.data(), nullptr) == ORBGPU_ERR_ARG);
    {
        orbgpu_covis_graph g = graph;
        g.n_kf = n_kf + 1;
        EXPECT(cullf(n, jobs.data(), &mirror, &ba, &cull, &g, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    }
    for (size_t off : {offsetof(orbgpu_map_mirror_ba, kf_first), offsetof(orbgpu_map_mirror_ba, kp_obs),
                       offsetof(orbgpu_map_mirror_ba, obs_idx)}) {
        orbgpu_map_mirror_ba b = ba;
        std::memset(reinterpret_cast<char*>(&b) + off, 0, sizeof(void*));
        EXPECT(cullf(n, jobs.data(), &mirror, &b, &cull, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    }
    for (size_t off = 0; off < sizeof(orbgpu_map_mirror_cull); off += sizeof(void*)) {
        orbgpu_map_mirror_cull c = cull;
        std::memset(reinterpret_cast<char*>(&c) + off, 0, sizeof(void*));
        EXPECT(cullf(n, jobs.data(), &mirror, &ba, &c, &graph, list_stride, cres.data(), verdicts.data(), culled.data()) == ORBGPU_ERR_ARG);
    }
    std::printf("ok\n");
    return 0;
}
