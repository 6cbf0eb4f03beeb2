// covis_args_main.cpp -- the host side of csrc/covis.hip on its own, for tests/test_covis.py: the argument
// checks of the erasure (every one comes before the device is looked at), compiled for the host under the
// address and undefined-behaviour sanitizers.  No HIP runtime is linked: the few names the host code refers
// to are defined here, and the device check answers that there is no device, so nothing is launched.
//   covis_args_main          runs the checks, prints "ok"
//   covis_args_main sizes    prints the size of orbgpu_covis_graph and some offsets
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

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

#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "covis_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static int sizes() {
    std::printf("orbgpu_covis_graph %zu\n", sizeof(orbgpu_covis_graph));
    std::printf("graph.conn_stride %zu\n", offsetof(orbgpu_covis_graph, conn_stride));
    std::printf("graph.n_conn %zu\n", offsetof(orbgpu_covis_graph, n_conn));
    std::printf("graph.ord_kf %zu\n", offsetof(orbgpu_covis_graph, ord_kf));
    std::printf("graph.covis10 %zu\n", offsetof(orbgpu_covis_graph, covis10));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    char block[256];
    void* p = block;  // never dereferenced: every call below returns before the device is looked at, or finds none
    auto ip = static_cast<int*>(p);
    auto cip = static_cast<const int*>(p);
    orbgpu_covis_graph graph;
    graph.n_kf = 4;
    graph.conn_stride = 8;
    graph.n_conn = graph.conn_kf = graph.conn_w = graph.n_ord = graph.ord_kf = graph.ord_w = graph.covis10 = ip;

    EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &graph, ip, nullptr) == ORBGPU_ERR_NO_DEVICE);  // valid: the device check
    EXPECT(orbgpu_covis_erase_keyframes_batch_device(-1, cip, &graph, ip, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, nullptr, &graph, ip, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, nullptr, ip, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &graph, nullptr, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(orbgpu_covis_erase_keyframes_batch_device(0, nullptr, nullptr, nullptr, nullptr) == ORBGPU_OK);  // nothing to do
    EXPECT(orbgpu_covis_erase_keyframes_batch_device(0, nullptr, &graph, nullptr, nullptr) == ORBGPU_OK);
    for (size_t off = offsetof(orbgpu_covis_graph, n_conn); off < sizeof(orbgpu_covis_graph); off += sizeof(void*)) {
        orbgpu_covis_graph g = graph;
        std::memset(reinterpret_cast<char*>(&g) + off, 0, sizeof(void*));
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_ARG);
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(0, nullptr, &g, nullptr, nullptr) == ORBGPU_ERR_ARG);  // a graph given is checked
    }
    for (int stride : {0, -3, ORBGPU_COVIS_MAX_STRIDE + 1}) {
        orbgpu_covis_graph g = graph;
        g.conn_stride = stride;
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_ARG);
    }
    {
        orbgpu_covis_graph g = graph;
        g.conn_stride = ORBGPU_COVIS_MAX_STRIDE;
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_NO_DEVICE);
        g.n_kf = -1;
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_ARG);
        g.n_kf = 1 << 22;  // n_kf * conn_stride does not fit an int
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_ARG);
        g.n_kf = (1 << 21) - 1;
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_NO_DEVICE);
    }
    {
        orbgpu_covis_graph g;  // no keyframes: every array may be NULL
        std::memset(&g, 0, sizeof(g));
        g.conn_stride = 1;
        EXPECT(orbgpu_covis_erase_keyframes_batch_device(1, cip, &g, ip, nullptr) == ORBGPU_ERR_NO_DEVICE);
    }
    std::printf("ok\n");
    return 0;
}
