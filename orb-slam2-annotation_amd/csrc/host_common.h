// host_common.h -- what the host translation units of liborbgpu.so share:
// error reporting and device checks (host_common.cpp), owning holders of HIP
// handles, and the one reader of the ORBGPU_* environment knobs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "../../include/orbgpu.h"

#define ORB_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return ::orbgpu::fail(ORBGPU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace orbgpu {

// thread-local message returned by orbgpu_last_error()
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
// ORBGPU_OK when the current HIP device is a gfx950, else ORBGPU_ERR_NO_DEVICE
int check_device();
// ORBGPU_ERR_ARG for a negative ordinal or one >= the visible device count,
// ORBGPU_ERR_NO_DEVICE when no device is visible
int validate_device(int device);

// The argument checks of a batch entry point whose jobs own ranges of shared per-item arrays
// (poseopt.hip, sim3opt.hip), made before the device is looked at; no pointer is dereferenced.
// `total_name` and `noun` are the entry point's words for the arrays' length and their items.
inline int check_batch_args(int batch, int total, const char* total_name, bool jobs_and_results, bool arrays,
                            const char* noun) {
    if (batch < 0 || total < 0) return fail(ORBGPU_ERR_ARG, std::string("negative batch or ") + total_name);
    if (batch > 0 && !jobs_and_results) return fail(ORBGPU_ERR_ARG, "null jobs or results");
    if (batch > 0 && total > 0 && !arrays) return fail(ORBGPU_ERR_ARG, std::string("null ") + noun + " array");
    return ORBGPU_OK;
}
// every job's [offset, offset + n) lies in [0, total); `jobs` is host memory
template <class Job>
int check_job_ranges(int batch, const Job* jobs, int total) {
    for (int b = 0; b < batch; ++b) {
        const Job& j = jobs[b];
        if (j.n < 0 || j.offset < 0 || (long long)j.offset + j.n > (long long)total)
            return fail(ORBGPU_ERR_ARG, "job " + std::to_string(b) + " is out of the array bounds");
    }
    return ORBGPU_OK;
}

// Makes `device` the calling thread's current HIP device for the scope and
// restores the previous one (device < 0: leaves the thread's device alone).
// Every entry point that takes an extractor runs under the extractor's device,
// so a handle created on GPU k works from any thread (orbgpu_extractor_create_on_device).
class DeviceScope {
  public:
    explicit DeviceScope(int device) {
        int cur = -1;
        if (device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess)
            prev_ = cur;
    }
    ~DeviceScope() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;

  private:
    int prev_ = -1;
};

// Move-only owner of one HIP handle, released when the owner goes.  It converts
// to the raw handle (what the launchers take); put() is the out-parameter of
// the creating call (hipMalloc, hipStreamCreate, ...).
template <class H, class Arg, hipError_t (*Release)(Arg)>
class Owned {
  public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.release()) {}
    Owned& operator=(Owned&& o) noexcept { reset(o.release()); return *this; }
    ~Owned() { reset(); }
    H get() const { return h_; }
    operator H() const { return h_; }
    H* put() { reset(); return &h_; }
    H release() { H h = h_; h_ = nullptr; return h; }
    void reset(H h = nullptr) { if (h_) (void)Release(h_); h_ = h; }

  private:
    H h_ = nullptr;
};
template <class T> using DevBuf = Owned<T*, void*, hipFree>;      // hipMalloc, hipExtMallocWithFlags
template <class T> using PinBuf = Owned<T*, void*, hipHostFree>;  // hipHostMalloc
using Stream = Owned<hipStream_t, hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEvent_t, hipEventDestroy>;

// `count` elements of HBM (at least one, so the pointer is never null)
template <class T>
int dalloc(DevBuf<T>& p, size_t count) {
    if (count == 0) count = 1;
    ORB_HIP(hipMalloc((void**)p.put(), count * sizeof(T)));
    return ORBGPU_OK;
}

// The ORBGPU_* environment knobs: atoi of the variable, `def` when it is unset;
// ranges are clamped where the knob is used.  env_now_int reads the environment
// at every call -- for the knobs a test switches within one process, and only
// those.  ORB_ENV_ONCE_INT / _FLAG read it at their first evaluation and keep
// that value for the process (a flag is off only when set to 0).
inline int env_now_int(const char* name, int def) {
    const char* s = std::getenv(name);
    return s ? std::atoi(s) : def;
}
#define ORB_ENV_ONCE_INT(name, def) \
    ([] { static const int v_ = ::orbgpu::env_now_int(name, def); return v_; }())
#define ORB_ENV_ONCE_FLAG(name, default_on) (ORB_ENV_ONCE_INT(name, (default_on) ? 1 : 0) != 0)

}  // namespace orbgpu
