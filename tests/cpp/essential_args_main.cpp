// essential_args_main.cpp -- the host side of csrc/essential.hip on its own, for tests/test_essential.py:
// the argument checks of both forms (every one comes before the device is looked at), the index checks
// of the host form and the workspace layout, compiled for the host under the address and
// undefined-behaviour sanitizers.  No HIP runtime is linked: the few names the host code refers to are
// defined here, and the device check answers that there is no device, so nothing is launched.
//   essential_args_main          runs the checks, prints "ok"
//   essential_args_main sizes    prints the size of orbgpu_eg_result and some offsets
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/essential.hip"

// ---- what liborbgpu.so and the HIP runtime would provide
namespace orbgpu {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int check_device() { return fail(ORBGPU_ERR_NO_DEVICE, "no device"); }
int host_ctx(HostCtx**) { return fail(ORBGPU_ERR_NO_DEVICE, "no device"); }
HostCtx::~HostCtx() {}
int HostCtx::reserve(size_t) { return fail(ORBGPU_ERR_NO_DEVICE, "no device"); }
hipError_t launch_copy16(void*, const void*, size_t, hipStream_t) { return hipErrorNoDevice; }
}  // namespace orbgpu

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "no HIP runtime"; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipHostMalloc(void**, size_t, unsigned int) { return hipErrorNoDevice; }
hipError_t hipHostFree(void*) { return hipSuccess; }
hipError_t hipMalloc(void**, size_t) { return hipErrorNoDevice; }
hipError_t hipFree(void*) { return hipSuccess; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipErrorNoDevice; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipErrorNoDevice; }
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { return nullptr; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "essential_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static int sizes() {
    std::printf("orbgpu_eg_result %zu\n", sizeof(orbgpu_eg_result));
    std::printf("result.n_active_edges %zu\n", offsetof(orbgpu_eg_result, n_active_edges));
    std::printf("result.first_chi2 %zu\n", offsetof(orbgpu_eg_result, first_chi2));
    std::printf("result.last_lambda %zu\n", offsetof(orbgpu_eg_result, last_lambda));
    return 0;
}

struct Call {  // the arguments of either form; a test changes one
    int N = 4, E = 5, M = 3, it = 5;
    // Tcw has_corrected Scorrected has_noncorrected Snoncorrected fixed | edge_i edge_j edge_kind | Xw point_ref |
    // Scw_out Tcw_out | Xw_out
    void* arr[14];
    orbgpu_eg_result* res;
    void* ws;
    size_t ws_bytes = size_t(1) << 40;
};

static int device_form(const Call& c) {
    return orbgpu_optimize_essential_graph_device(
        c.N, c.E, c.M, (const float*)c.arr[0], (const uint8_t*)c.arr[1], (const double*)c.arr[2],
        (const uint8_t*)c.arr[3], (const double*)c.arr[4], (const uint8_t*)c.arr[5], (const int*)c.arr[6],
        (const int*)c.arr[7], (const uint8_t*)c.arr[8], (const float*)c.arr[9], (const int*)c.arr[10], 1, c.it,
        (double*)c.arr[11], (float*)c.arr[12], (float*)c.arr[13], c.res, c.ws, c.ws_bytes, nullptr);
}
static int host_form(const Call& c) {
    return orbgpu_optimize_essential_graph(
        c.N, c.E, c.M, (const float*)c.arr[0], (const uint8_t*)c.arr[1], (const double*)c.arr[2],
        (const uint8_t*)c.arr[3], (const double*)c.arr[4], (const uint8_t*)c.arr[5], (const int*)c.arr[6],
        (const int*)c.arr[7], (const uint8_t*)c.arr[8], (const float*)c.arr[9], (const int*)c.arr[10], 1, c.it,
        (double*)c.arr[11], (float*)c.arr[12], (float*)c.arr[13], c.res, c.ws, c.ws_bytes);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    alignas(8) char block[256];
    int edge_i[5] = {1, 2, 3, 3, 0}, edge_j[5] = {0, 1, 2, 0, 2}, point_ref[3] = {0, -1, 3};
    orbgpu_eg_result res;
    Call ok;
    for (void*& p : ok.arr) p = block;  // never dereferenced, the three index arrays of the host form aside
    ok.arr[6] = edge_i, ok.arr[7] = edge_j, ok.arr[10] = point_ref;
    ok.res = &res, ok.ws = block;
    for (int form = 0; form < 2; ++form) {
        auto call = form ? host_form : device_form;
        EXPECT(call(ok) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
        for (int which = 0; which < 4; ++which) {
            Call c = ok;
            (which == 0 ? c.N : which == 1 ? c.E : which == 2 ? c.M : c.it) = -1;
            EXPECT(call(c) == ORBGPU_ERR_ARG);
        }
        for (int k = 0; k < 14; ++k) {
            Call c = ok;
            c.arr[k] = nullptr;
            EXPECT(call(c) == ORBGPU_ERR_ARG);
        }
        Call c = ok;
        c.res = nullptr;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c = ok;
        c.ws = block + 4;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c = ok;
        c.ws_bytes = orbgpu_essential_graph_workspace_bytes(4, 5, 3) - 1;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c.ws_bytes += 1;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c = ok;  // a NULL array is fine where its count is zero
        c.E = 0, c.M = 0;
        for (int k : {6, 7, 8, 9, 10, 13}) c.arr[k] = nullptr;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c = ok;
        c.N = INT_MAX;  // the dense system does not fit a size_t
        EXPECT(call(c) == ORBGPU_ERR_ARG);
    }
    {  // the device form takes no NULL workspace; the host form allocates its own, after the device check
        Call c = ok;
        c.ws = nullptr;
        EXPECT(device_form(c) == ORBGPU_ERR_ARG && host_form(c) == ORBGPU_ERR_NO_DEVICE);
    }
    // the host form reads every edge index, i != j and every point_ref; the device form leaves them to a kernel
    const int bad[][3] = {{6, 2, 4}, {6, 0, -1}, {7, 4, INT_MAX}, {7, 1, INT_MIN}, {7, 3, 3}, {10, 2, 4}, {10, 0, INT_MAX}};
    for (auto& b : bad) {
        int ei[5], ej[5], pr[3];
        std::memcpy(ei, edge_i, sizeof(ei)), std::memcpy(ej, edge_j, sizeof(ej)), std::memcpy(pr, point_ref, sizeof(pr));
        (b[0] == 6 ? ei : b[0] == 7 ? ej : pr)[b[1]] = b[2];
        Call c = ok;
        c.arr[6] = ei, c.arr[7] = ej, c.arr[10] = pr;
        EXPECT(host_form(c) == ORBGPU_ERR_ARG && device_form(c) == ORBGPU_ERR_NO_DEVICE);
    }
    {  // any negative point_ref keeps the point
        int pr[3] = {INT_MIN, -1, 3};
        Call c = ok;
        c.arr[10] = pr;
        EXPECT(host_form(c) == ORBGPU_ERR_NO_DEVICE);
    }
    // the layout: sizes grow with every count, are multiples of 8, and 0 stands for what does not fit
    size_t prev = 0;
    for (int n = 0; n <= 640; n += 80) {
        const size_t a = orbgpu_essential_graph_workspace_bytes(n, 12 * n, 500 * n);
        EXPECT(a > prev && a % 8 == 0);
        const Layout l = make_layout(n, 12 * n);
        EXPECT(l.bytes == a && l.ints + 4 * (l.list_i + 2 * l.E) <= a);
        EXPECT(kCtlBytes + 8 * (l.scale_d + l.n_scale) == l.ints);
        EXPECT(l.x_d == l.sys_d + (7 * (size_t)n + 1) * 7 * (size_t)n);
        EXPECT(l.edge_d == (size_t)kVertD * n && l.sys_d == l.edge_d + (size_t)kEdgeD * 12 * n);
        prev = a;
    }
    EXPECT(orbgpu_essential_graph_workspace_bytes(-1, 0, 0) == 0 && orbgpu_essential_graph_workspace_bytes(0, -1, 0) == 0);
    EXPECT(orbgpu_essential_graph_workspace_bytes(0, 0, -1) == 0);
    EXPECT(orbgpu_essential_graph_workspace_bytes(INT_MAX, INT_MAX, INT_MAX) == 0);
    EXPECT(orbgpu_essential_graph_workspace_bytes(0, INT_MAX, INT_MAX) > 0);
    std::printf("ok\n");
    return 0;
}
