// localba_chip_args_main.cpp -- the host side of csrc/localba_chip.hip on its own, for
// tests/test_localba_chip.py: the argument checks of both forms (every one comes before the device is
// looked at), the edge index checks of the host form and the workspace layout, compiled for the host
// under the address and undefined-behaviour sanitizers.  No HIP runtime is linked: the few names the
// host code refers to are defined here, and the device check answers that there is no device, so
// nothing is launched.
//   localba_chip_args_main          runs the checks, prints "ok"
//   localba_chip_args_main sizes    prints the size of orbgpu_localba_chip_result and its offsets
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/localba_chip.hip"

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

#define EXPECT(cond)                                                                      \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "localba_chip_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int sizes() {
    typedef orbgpu_localba_chip_result R;
    std::printf("orbgpu_localba_chip_result %zu\n", sizeof(R));
    std::printf("status %zu\nrounds %zu\nn_bad_first %zu\nn_erase %zu\nstop_poll %zu\npolls %zu\n", offsetof(R, status),
                offsetof(R, rounds), offsetof(R, n_bad_first), offsetof(R, n_erase), offsetof(R, stop_poll),
                offsetof(R, polls));
    std::printf("lm_iterations %zu\nlm_rejected %zu\nstopped %zu\niterations_applied %zu\nn_free %zu\nn_active_points %zu\n",
                offsetof(R, lm_iterations), offsetof(R, lm_rejected), offsetof(R, stopped),
                offsetof(R, iterations_applied), offsetof(R, n_free), offsetof(R, n_active_points));
    return 0;
}

struct Call {  // the arguments of either form; a test changes one
    int P = 3, NL = 2, M = 4, E = 6, it1 = 5, it2 = 10, stop_at = -1;
    void* arr[11];  // Tcw fixed cam Xw edge_pose edge_point obs inv_sigma2 Tcw_out Xw_out erase
    orbgpu_localba_chip_result* res;
    void* ws;
    size_t ws_bytes = size_t(1) << 40;
};

static int device_form(const Call& c) {
    return orbgpu_local_ba_chip_device(
        c.P, c.NL, c.M, c.E, (const float*)c.arr[0], (const uint8_t*)c.arr[1], (const float*)c.arr[2],
        (const float*)c.arr[3], (const int*)c.arr[4], (const int*)c.arr[5], (const float*)c.arr[6],
        (const float*)c.arr[7], c.it1, c.it2, nullptr, c.stop_at, (float*)c.arr[8], (float*)c.arr[9],
        (uint8_t*)c.arr[10], c.res, c.ws, c.ws_bytes, nullptr);
}
static int host_form(const Call& c) {
    return orbgpu_local_ba_chip(
        c.P, c.NL, c.M, c.E, (const float*)c.arr[0], (const uint8_t*)c.arr[1], (const float*)c.arr[2],
        (const float*)c.arr[3], (const int*)c.arr[4], (const int*)c.arr[5], (const float*)c.arr[6],
        (const float*)c.arr[7], c.it1, c.it2, nullptr, c.stop_at, (float*)c.arr[8], (float*)c.arr[9],
        (uint8_t*)c.arr[10], c.res, c.ws, c.ws_bytes);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    alignas(8) char block[256];
    int edge_pose[6] = {0, 1, 2, 0, 1, 2}, edge_point[6] = {0, 0, 1, 2, 3, 3};
    orbgpu_localba_chip_result res;
    Call ok;
    for (void*& p : ok.arr) p = block;  // never dereferenced, the two index arrays of the host form aside
    ok.arr[4] = edge_pose, ok.arr[5] = edge_point;
    ok.res = &res, ok.ws = block;
    for (int form = 0; form < 2; ++form) {
        auto call = form ? host_form : device_form;
        EXPECT(call(ok) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
        for (int which = 0; which < 6; ++which) {
            Call c = ok;
            (which == 0 ? c.P : which == 1 ? c.NL : which == 2 ? c.M : which == 3 ? c.E : which == 4 ? c.it1 : c.it2) = -1;
            EXPECT(call(c) == ORBGPU_ERR_ARG);
        }
        Call c = ok;
        c.NL = c.P + 1;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c.NL = c.P;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c = ok;
        c.stop_at = -2;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c.stop_at = 0;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c.stop_at = INT_MAX;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        for (int k = 0; k < 11; ++k) {
            c = ok;
            c.arr[k] = nullptr;
            EXPECT(call(c) == ORBGPU_ERR_ARG);
        }
        c = ok;
        c.res = nullptr;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c = ok;
        c.ws = block + 4;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c = ok;
        c.ws_bytes = orbgpu_local_ba_chip_workspace_bytes(3, 2, 4, 6) - 1;
        EXPECT(call(c) == ORBGPU_ERR_ARG);
        c.ws_bytes += 1;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c = ok;  // a NULL array is fine where its count is zero
        c.M = 0, c.E = 0, c.arr[3] = c.arr[9] = c.arr[10] = nullptr;
        for (int k = 4; k < 8; ++k) c.arr[k] = nullptr;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c = ok;  // no local pose: no pose output
        c.NL = 0, c.arr[8] = nullptr;
        EXPECT(call(c) == ORBGPU_ERR_NO_DEVICE);
        c = ok;
        c.P = c.NL = INT_MAX;  // the dense reduced system does not fit a size_t
        EXPECT(call(c) == ORBGPU_ERR_ARG);
    }
    {  // the device form takes no NULL workspace; the host form allocates its own, after the device check
        Call c = ok;
        c.ws = nullptr;
        EXPECT(device_form(c) == ORBGPU_ERR_ARG && host_form(c) == ORBGPU_ERR_NO_DEVICE);
    }
    // the host form reads every edge index and the order of edge_point
    const int bad_pose[][2] = {{2, 3}, {2, -1}, {5, INT_MAX}}, bad_point[][2] = {{5, 4}, {0, -1}, {3, 0}, {1, INT_MIN}};
    for (auto& b : bad_pose) {
        int ep[6];
        std::memcpy(ep, edge_pose, sizeof(ep));
        ep[b[0]] = b[1];
        Call c = ok;
        c.arr[4] = ep;
        EXPECT(host_form(c) == ORBGPU_ERR_ARG && device_form(c) == ORBGPU_ERR_NO_DEVICE);
    }
    for (auto& b : bad_point) {
        int el[6];
        std::memcpy(el, edge_point, sizeof(el));
        el[b[0]] = b[1];
        Call c = ok;
        c.arr[5] = el;
        EXPECT(host_form(c) == ORBGPU_ERR_ARG);
    }
    // the layout: sizes grow with every count, are multiples of 8, and 0 stands for what does not fit
    size_t prev = 0;
    for (int n = 0; n <= 640; n += 80) {
        const size_t a = orbgpu_local_ba_chip_workspace_bytes(2 * n, n, 100 * n, 500 * n);
        EXPECT(a > prev && a % 8 == 0);
        const Layout l = make_layout(2 * n, n, 100 * n, 500 * n);
        EXPECT(l.bytes == a && l.ints + 4 * (l.edge_i + kEdgeI * l.E) <= a);  // the list and the level words
        EXPECT(kCtlBytes + kCountBytes + 8 * (l.scale_d + l.n_scale) == l.ints);
        EXPECT(l.sys_d == l.edge_d + (size_t)kEdgeD * l.E);  // the last chi2 is the edges' last field
        EXPECT(l.x_d == l.sys_d + (6 * (size_t)n + 1) * 6 * (size_t)n);  // sized by the local poses alone
        prev = a;
    }
    EXPECT(orbgpu_local_ba_chip_workspace_bytes(50, 30, 0, 0) < orbgpu_local_ba_chip_workspace_bytes(50, 31, 0, 0));
    EXPECT(orbgpu_local_ba_chip_workspace_bytes(-1, 0, 0, 0) == 0 && orbgpu_local_ba_chip_workspace_bytes(1, -1, 0, 0) == 0);
    EXPECT(orbgpu_local_ba_chip_workspace_bytes(0, 0, -1, 0) == 0 && orbgpu_local_ba_chip_workspace_bytes(0, 0, 0, -1) == 0);
    EXPECT(orbgpu_local_ba_chip_workspace_bytes(2, 3, 0, 0) == 0);  // n_local > n_poses
    EXPECT(orbgpu_local_ba_chip_workspace_bytes(INT_MAX, INT_MAX, INT_MAX, INT_MAX) == 0);
    EXPECT(orbgpu_local_ba_chip_workspace_bytes(INT_MAX, 0, INT_MAX, INT_MAX) > 0);
    std::printf("ok\n");
    return 0;
}
