// reloc_args_main.cpp -- the host side of csrc/reloc.hip's entry points on its own, for
// tests/test_reloc.py: the argument checks (every one comes before the device is looked at) and the
// carving of both opaque blocks from a null base, compiled for the host under the address and
// undefined-behaviour sanitizers.  No HIP runtime is linked: the few names the host code refers to
// are defined here, and the device check answers that there is no device, so nothing is launched.
//   reloc_args_main          runs the checks, prints "ok"
//   reloc_args_main sizes    prints the size of every struct of orbgpu_reloc.h and some offsets
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/reloc.hip"

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
size_t orbgpu_pnp_workspace_bytes(int total_points, int total_samples) {
    return (size_t)(total_points > 0 ? total_points : 1) * 4 + (size_t)(total_samples > 0 ? total_samples : 1) * 104;
}
int orbgpu_pnp_ransac_batch_device(int, const orbgpu_pnp_problem*, int, int, int, const float*, const float*,
                                   const float*, const int*, void*, orbgpu_pnp_result*, uint8_t*, uint8_t*, void*) {
    return ORBGPU_ERR_NO_DEVICE;
}
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
            std::fprintf(stderr, "reloc_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static int sizes() {
    std::printf("orbgpu_reloc_frame %zu\n", sizeof(orbgpu_reloc_frame));
    std::printf("orbgpu_reloc_candidate %zu\n", sizeof(orbgpu_reloc_candidate));
    std::printf("orbgpu_reloc_query %zu\n", sizeof(orbgpu_reloc_query));
    std::printf("orbgpu_relocalize_result %zu\n", sizeof(orbgpu_relocalize_result));
    std::printf("orbgpu_reloc_candidate_state %zu\n", sizeof(orbgpu_reloc_candidate_state));
    std::printf("frame.level_sigma2 %zu\n", offsetof(orbgpu_reloc_frame, level_sigma2));
    std::printf("result.nadditional %zu\n", offsetof(orbgpu_relocalize_result, nadditional));
    std::printf("result.pnp_Tcw %zu\n", offsetof(orbgpu_relocalize_result, pnp_Tcw));
    std::printf("result.Tcw %zu\n", offsetof(orbgpu_relocalize_result, Tcw));
    std::printf("result.opt %zu\n", offsetof(orbgpu_relocalize_result, opt));
    std::printf("result.rng_after %zu\n", offsetof(orbgpu_relocalize_result, rng_after));
    std::printf("state.discarded %zu\n", offsetof(orbgpu_reloc_candidate_state, discarded));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    char block[256];
    void* p = block;  // never dereferenced: every call below returns before the device is looked at, or finds none
    auto q = static_cast<const orbgpu_reloc_query*>(p);
    auto c = static_cast<const orbgpu_reloc_candidate*>(p);
    auto f = static_cast<const orbgpu_reloc_frame*>(p);
    auto k = static_cast<const orbgpu_loop_keyframe*>(p);
    auto ks = static_cast<const orbgpu_loop_keyframe_search*>(p);
    auto ip = static_cast<int*>(p);
    auto res = static_cast<orbgpu_relocalize_result*>(p);
    auto st = static_cast<orbgpu_reloc_candidate_state*>(p);
    auto run = [&](int nq, int nc, int stride, int passes, int resume, void* state, int* rows) {
        return orbgpu_relocalize_batch_device(nq, q, nc, c, f, k, ks, ip, stride, p, passes, resume, state, res, st, rows,
                                              nullptr);
    };
    EXPECT(run(-1, 1, 8, 1, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, -1, 8, 1, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, 1, 0, 1, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, 1, 8, 0, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, 1, 8, 1, 2, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, 1, 8, 1, 0, nullptr, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, 1, 8, 1, 0, p, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(run(1 << 20, 1, 1 << 12, 1, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(1, 1 << 20, 1 << 12, 1, 0, p, ip) == ORBGPU_ERR_ARG);
    EXPECT(run(0, 0, 8, 1, 0, nullptr, nullptr) == ORBGPU_OK);
    EXPECT(run(1, 1, 8, 1, 0, p, ip) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
    auto setup = [&](int nc, int stride, void* ws) {
        return orbgpu_reloc_setup_batch_device(nc, c, f, k, ip, stride, ip, ws, ip, nullptr);
    };
    EXPECT(setup(-1, 8, p) == ORBGPU_ERR_ARG);
    EXPECT(setup(1, 0, p) == ORBGPU_ERR_ARG);
    EXPECT(setup(1, 8, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(setup(1 << 20, 1 << 12, p) == ORBGPU_ERR_ARG);
    EXPECT(setup(0, 8, nullptr) == ORBGPU_OK);
    EXPECT(setup(1, 8, p) == ORBGPU_ERR_NO_DEVICE);
    // the carving: sizes from a null base grow with every dimension and are 256-byte multiples
    size_t prev = 0;
    for (int n = 0; n <= 64; n += 8) {
        const size_t a = orbgpu_reloc_setup_workspace_bytes(n, 300), b = orbgpu_relocalize_workspace_bytes(n, 3 * n, 300);
        EXPECT(a > 0 && b > 0 && a % 256 == 0 && b % 256 == 0 && a + b >= prev);
        prev = a + b;
    }
    EXPECT(orbgpu_reloc_setup_workspace_bytes(-5, -5) == orbgpu_reloc_setup_workspace_bytes(1, 1));
    EXPECT(orbgpu_relocalize_workspace_bytes(1, 1 << 20, 1 << 12) == 0);  // n_cand * stride does not fit an int
    std::printf("ok\n");
    return 0;
}
