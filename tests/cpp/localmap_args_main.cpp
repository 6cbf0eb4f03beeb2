// localmap_args_main.cpp -- the host side of csrc/localmap.hip on its own, for tests/test_localmap.py:
// the argument checks (every one comes before the device is looked at) and the carving of the opaque
// block from a null base, compiled for the host under the address and undefined-behaviour sanitizers.
// No HIP runtime is linked: the few names the host code refers to are defined here, and the device
// check answers that there is no device, so nothing is launched.
//   localmap_args_main          runs the checks, prints "ok"
//   localmap_args_main sizes    prints the size of every struct of orbgpu_localmap.h and some offsets
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/localmap.hip"

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

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "localmap_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static int sizes() {
    std::printf("orbgpu_map_mirror %zu\n", sizeof(orbgpu_map_mirror));
    std::printf("orbgpu_update_local_map_job %zu\n", sizeof(orbgpu_update_local_map_job));
    std::printf("orbgpu_update_local_map_result %zu\n", sizeof(orbgpu_update_local_map_result));
    std::printf("mirror.kf_bad %zu\n", offsetof(orbgpu_map_mirror, kf_bad));
    std::printf("mirror.kf_by_rank %zu\n", offsetof(orbgpu_map_mirror, kf_by_rank));
    std::printf("mirror.obs %zu\n", offsetof(orbgpu_map_mirror, obs));
    std::printf("mirror.max_dist %zu\n", offsetof(orbgpu_map_mirror, max_dist));
    std::printf("job.rows %zu\n", offsetof(orbgpu_update_local_map_job, rows));
    std::printf("job.prev_kfs %zu\n", offsetof(orbgpu_update_local_map_job, prev_kfs));
    std::printf("job.out_desc %zu\n", offsetof(orbgpu_update_local_map_job, out_desc));
    std::printf("job.local_job %zu\n", offsetof(orbgpu_update_local_map_job, local_job));
    std::printf("result.ref_kf %zu\n", offsetof(orbgpu_update_local_map_result, ref_kf));
    std::printf("result.n_extra %zu\n", offsetof(orbgpu_update_local_map_result, n_extra));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    char block[256];
    void* p = block;  // never dereferenced: every call below returns before the device is looked at, or finds none
    auto jobs = static_cast<const orbgpu_update_local_map_job*>(p);
    auto res = static_cast<orbgpu_update_local_map_result*>(p);
    auto ip = static_cast<int*>(p);
    auto cip = static_cast<const int*>(p);
    auto cfp = static_cast<const float*>(p);
    auto cbp = static_cast<const uint8_t*>(p);
    orbgpu_map_mirror full;
    std::memset(&full, 0, sizeof(full));
    full.n_kf = 4;
    full.n_pt = 9;
    full.n_slots_total = 12;
    full.n_children_total = 2;
    full.n_obs_total = 12;
    full.kf_bad = cbp;
    full.slot_offset = full.n_slots = full.slots = full.covis = full.child_offset = full.n_children = full.children =
        full.parent = cip;
    full.pt_flags = full.obs_offset = full.n_obs = full.obs = cip;
    full.pos = full.normal = full.min_dist = full.max_dist = cfp;
    full.desc = cbp;
    auto call = [&](int n, const orbgpu_map_mirror* m, int stride, int ps, int ks, void* ws, int* kfs, int* pts) {
        return orbgpu_update_local_map_batch_device(n, jobs, m, stride, ps, ks, ws, res, kfs, pts, nullptr);
    };
    EXPECT(call(1, &full, 8, 8, 8, p, ip, ip) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
    EXPECT(call(-1, &full, 8, 8, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 0, 8, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 8, 0, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 8, 8, 0, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 8, 8, 65536, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, nullptr, 8, 8, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 8, 8, 8, nullptr, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 8, 8, 8, p, nullptr, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, &full, 8, 8, 8, p, ip, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(orbgpu_update_local_map_batch_device(1, nullptr, &full, 8, 8, 8, p, res, ip, ip, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(orbgpu_update_local_map_batch_device(1, jobs, &full, 8, 8, 8, p, nullptr, ip, ip, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(call(1 << 20, &full, 1 << 12, 8, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1 << 20, &full, 8, 1 << 12, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1 << 20, &full, 8, 8, 1 << 12, p, ip, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(0, nullptr, 8, 8, 8, nullptr, nullptr, nullptr) == ORBGPU_OK);  // nothing to do: no device needed
    // the mirror: negative counts, and NULL arrays with positive counts
    for (int which = 0; which < 5; ++which) {
        orbgpu_map_mirror m = full;
        (which == 0 ? m.n_kf : which == 1 ? m.n_pt : which == 2 ? m.n_slots_total : which == 3 ? m.n_children_total
                                                                                              : m.n_obs_total) = -1;
        EXPECT(call(1, &m, 8, 8, 8, p, ip, ip) == ORBGPU_ERR_ARG);
    }
    const size_t first = offsetof(orbgpu_map_mirror, kf_bad);
    for (size_t off = first; off < sizeof(orbgpu_map_mirror); off += sizeof(void*)) {
        orbgpu_map_mirror m = full;
        std::memset(reinterpret_cast<char*>(&m) + off, 0, sizeof(void*));
        const int want = off == offsetof(orbgpu_map_mirror, kf_by_rank) ? ORBGPU_ERR_NO_DEVICE : ORBGPU_ERR_ARG;
        EXPECT(call(1, &m, 8, 8, 8, p, ip, ip) == want);
    }
    orbgpu_map_mirror empty;  // no keyframes, no points: every array may be NULL
    std::memset(&empty, 0, sizeof(empty));
    EXPECT(call(1, &empty, 8, 8, 8, p, ip, ip) == ORBGPU_ERR_NO_DEVICE);
    // the carving: sizes from a null base grow with every dimension and are 256-byte multiples
    size_t prev = 0;
    for (int n = 0; n <= 64; n += 8) {
        const size_t a = orbgpu_update_local_map_workspace_bytes(n, 300, 40 * n, 16 + n, 10 * n, 100 * n);
        EXPECT(a > 0 && a % 256 == 0 && a >= prev);
        prev = a;
    }
    EXPECT(orbgpu_update_local_map_workspace_bytes(-5, -5, -5, -5, -5, -5) ==
           orbgpu_update_local_map_workspace_bytes(1, 1, 1, 1, 1, 1));
    EXPECT(orbgpu_update_local_map_workspace_bytes(2, 8, 8, 8, 0, 0) == orbgpu_update_local_map_workspace_bytes(2, 8, 8, 8, 1, 1));
    EXPECT(orbgpu_update_local_map_workspace_bytes(1 << 20, 8, 8, 1 << 12, 4, 4) == 0);  // n * kf_stride does not fit an int
    std::printf("ok\n");
    return 0;
}
