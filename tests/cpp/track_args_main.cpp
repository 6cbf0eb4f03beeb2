// track_args_main.cpp -- the host side of csrc/track.hip's three entry points on its own, for
// tests/test_track.py: the argument checks (every one comes before the device is looked at) and the
// carving of both opaque blocks from a null base, compiled for the host under the address and
// undefined-behaviour sanitizers.  No HIP runtime is linked: the few names the host code refers to
// are defined here, and the device check answers that there is no device, so nothing is launched.
//   track_args_main          runs the checks, prints "ok"
//   track_args_main sizes    prints the size of every struct of orbgpu_track.h and some offsets
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/track.hip"

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
int orbgpu_pose_optimization_batch_device(int, const orbgpu_poseopt_job*, int, const float*, const float*, const float*,
                                          orbgpu_poseopt_result*, uint8_t*, void*) {
    return ORBGPU_ERR_NO_DEVICE;
}
int orbgpu_search_by_projection_batch_device(int, const orbgpu_proj_call*, int, int*, int*, void*) {
    return ORBGPU_ERR_NO_DEVICE;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "no HIP runtime"; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { return nullptr; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "track_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static int sizes() {
    std::printf("orbgpu_track_initial_job %zu\n", sizeof(orbgpu_track_initial_job));
    std::printf("orbgpu_track_initial_result %zu\n", sizeof(orbgpu_track_initial_result));
    std::printf("orbgpu_track_local_job %zu\n", sizeof(orbgpu_track_local_job));
    std::printf("orbgpu_track_local_result %zu\n", sizeof(orbgpu_track_local_result));
    std::printf("orbgpu_update_last_frame_job %zu\n", sizeof(orbgpu_update_last_frame_job));
    std::printf("orbgpu_update_last_frame_result %zu\n", sizeof(orbgpu_update_last_frame_result));
    std::printf("initial_job.Tcw_init %zu\n", offsetof(orbgpu_track_initial_job, Tcw_init));
    std::printf("initial_job.points %zu\n", offsetof(orbgpu_track_initial_job, points));
    std::printf("initial_job.bow_nmatches %zu\n", offsetof(orbgpu_track_initial_job, bow_nmatches));
    std::printf("initial_result.opt %zu\n", offsetof(orbgpu_track_initial_result, opt));
    std::printf("initial_result.Tcw %zu\n", offsetof(orbgpu_track_initial_result, Tcw));
    std::printf("local_job.Tcw %zu\n", offsetof(orbgpu_track_local_job, Tcw));
    std::printf("local_job.points %zu\n", offsetof(orbgpu_track_local_job, points));
    std::printf("local_result.Tcw %zu\n", offsetof(orbgpu_track_local_result, Tcw));
    std::printf("update_job.Rwc %zu\n", offsetof(orbgpu_update_last_frame_job, Rwc));
    std::printf("update_job.flags %zu\n", offsetof(orbgpu_update_last_frame_job, flags));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    char block[256];
    void* p = block;  // never dereferenced: every call below returns before the device is looked at, or finds none
    auto ij = static_cast<const orbgpu_track_initial_job*>(p);
    auto lj = static_cast<const orbgpu_track_local_job*>(p);
    auto uj = static_cast<const orbgpu_update_last_frame_job*>(p);
    auto f = static_cast<const orbgpu_reloc_frame*>(p);
    auto ir = static_cast<orbgpu_track_initial_result*>(p);
    auto lr = static_cast<orbgpu_track_local_result*>(p);
    auto ur = static_cast<orbgpu_update_last_frame_result*>(p);
    auto ip = static_cast<int*>(p);
    auto bp = static_cast<uint8_t*>(p);
    auto initial = [&](int n, int nf, int stride, void* ws, int* rows) {
        return orbgpu_track_initial_batch_device(n, ij, nf, f, stride, ws, ir, rows, nullptr);
    };
    EXPECT(initial(-1, 1, 8, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(initial(1, -1, 8, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(initial(1, 1, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(initial(1, 1, 8, nullptr, ip) == ORBGPU_ERR_ARG);
    EXPECT(initial(1, 1, 8, p, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(initial(1 << 20, 1, 1 << 12, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(initial(0, 0, 8, nullptr, nullptr) == ORBGPU_OK);
    EXPECT(initial(1, 1, 8, p, ip) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
    auto local = [&](int n, int nf, int stride, int ps, void* ws, uint8_t* flags) {
        return orbgpu_track_local_map_batch_device(n, lj, nf, f, stride, ps, ws, lr, ip, flags, nullptr);
    };
    EXPECT(local(-1, 1, 8, 8, p, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(1, -1, 8, 8, p, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(1, 1, 0, 8, p, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(1, 1, 8, 0, p, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(1, 1, 8, 8, nullptr, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(1, 1, 8, 8, p, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(local(1 << 20, 1, 1 << 12, 8, p, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(1 << 20, 1, 8, 1 << 12, p, bp) == ORBGPU_ERR_ARG);
    EXPECT(local(0, 0, 8, 8, nullptr, nullptr) == ORBGPU_OK);
    EXPECT(local(1, 1, 8, 8, p, bp) == ORBGPU_ERR_NO_DEVICE);
    auto update = [&](int n, int stride, uint8_t* created) {
        return orbgpu_update_last_frame_batch_device(n, uj, stride, ur, created, nullptr);
    };
    EXPECT(update(-1, 8, bp) == ORBGPU_ERR_ARG);
    EXPECT(update(1, 0, bp) == ORBGPU_ERR_ARG);
    EXPECT(update(1, 8, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(update(1 << 20, 1 << 12, bp) == ORBGPU_ERR_ARG);
    EXPECT(update(0, 8, nullptr) == ORBGPU_OK);
    EXPECT(update(1, 8, bp) == ORBGPU_ERR_NO_DEVICE);
    // the carving: sizes from a null base grow with every dimension and are 256-byte multiples
    size_t prev = 0;
    for (int n = 0; n <= 64; n += 8) {
        const size_t a = orbgpu_track_initial_workspace_bytes(n, 300), b = orbgpu_track_local_workspace_bytes(n, 300, 40 * n);
        EXPECT(a > 0 && b > 0 && a % 256 == 0 && b % 256 == 0 && a + b >= prev);
        prev = a + b;
    }
    EXPECT(orbgpu_track_initial_workspace_bytes(-5, -5) == orbgpu_track_initial_workspace_bytes(1, 1));
    EXPECT(orbgpu_track_local_workspace_bytes(-5, -5, -5) == orbgpu_track_local_workspace_bytes(1, 1, 1));
    EXPECT(orbgpu_track_initial_workspace_bytes(1 << 20, 1 << 12) == 0);  // n * stride does not fit an int
    EXPECT(orbgpu_track_local_workspace_bytes(1 << 20, 8, 1 << 12) == 0);
    std::printf("ok\n");
    return 0;
}
