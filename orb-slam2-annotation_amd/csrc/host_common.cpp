// host_common.cpp -- error reporting and device checks of host_common.h, and
// the C ABI's process-level entry points (include/orbgpu.h): last error, ABI
// version, device queries, the calling thread's device, device events.
// There is no CPU fallback: without a gfx950 device every entry point fails
// with ORBGPU_ERR_NO_DEVICE.
#include "host_common.h"

#include <cstring>

namespace orbgpu {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int check_device() {
    // the arch check once per device and thread (the host-form calls run it on every call)
    static thread_local int checked_dev = -1;
    int dev = 0, n = 0;
    if (checked_dev >= 0 && hipGetDevice(&dev) == hipSuccess && dev == checked_dev) return ORBGPU_OK;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ORBGPU_ERR_NO_DEVICE, "no HIP device visible");
    ORB_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    ORB_HIP(hipGetDeviceProperties(&p, dev));
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(ORBGPU_ERR_NO_DEVICE, std::string("device is ") + p.gcnArchName + ", this build targets gfx950");
    checked_dev = dev;
    return ORBGPU_OK;
}

int validate_device(int device) {
    if (device < 0) return fail(ORBGPU_ERR_ARG, "device ordinal must be >= 0");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ORBGPU_ERR_NO_DEVICE, "no HIP device visible");
    if (device >= n)
        return fail(ORBGPU_ERR_ARG, "device ordinal " + std::to_string(device) + " >= visible devices (" +
                                        std::to_string(n) + ")");
    return ORBGPU_OK;
}

}  // namespace orbgpu

using namespace orbgpu;

extern "C" {

const char* orbgpu_last_error(void) { return g_err.c_str(); }

int orbgpu_abi_version(void) { return ORBGPU_ABI_VERSION; }

int orbgpu_device_arch(char* buf, int buflen) {
    int dev = 0, n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ORBGPU_ERR_NO_DEVICE, "no HIP device visible");
    ORB_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    ORB_HIP(hipGetDeviceProperties(&p, dev));
    if (buf && buflen > 0) {
        std::strncpy(buf, p.gcnArchName, (size_t)buflen - 1);
        buf[buflen - 1] = 0;
    }
    return ORBGPU_OK;
}

int orbgpu_device_count(int* n) {
    if (!n) return fail(ORBGPU_ERR_ARG, "n is NULL");
    *n = 0;
    if (hipGetDeviceCount(n) != hipSuccess) *n = 0;
    return ORBGPU_OK;
}

int orbgpu_set_thread_device(int device) {
    int rc = validate_device(device);
    if (rc) return rc;
    ORB_HIP(hipSetDevice(device));
    return check_device();
}

int orbgpu_get_thread_device(int* device) {
    if (!device) return fail(ORBGPU_ERR_ARG, "device is NULL");
    *device = -1;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ORBGPU_ERR_NO_DEVICE, "no HIP device visible");
    ORB_HIP(hipGetDevice(device));
    return ORBGPU_OK;
}

int orbgpu_device_event_create(void** event) {
    if (!event) return fail(ORBGPU_ERR_ARG, "NULL event");
    hipEvent_t e = nullptr;
    ORB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    *event = e;
    return ORBGPU_OK;
}

int orbgpu_device_event_destroy(void* event) {
    if (event) ORB_HIP(hipEventDestroy((hipEvent_t)event));
    return ORBGPU_OK;
}

int orbgpu_device_event_record(void* event, void* stream) {
    if (!event) return fail(ORBGPU_ERR_ARG, "NULL event");
    ORB_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return ORBGPU_OK;
}

int orbgpu_stream_wait_device_event(void* stream, void* event) {
    if (!event) return fail(ORBGPU_ERR_ARG, "NULL event");
    ORB_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return ORBGPU_OK;
}

}  // extern "C"
