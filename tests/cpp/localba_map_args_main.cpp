// localba_map_args_main.cpp -- the host side of csrc/localba_map.hip on its own, for
// tests/test_localba_map.py: the argument checks of the gather and of the collection (every one comes
// before the device is looked at) and the carving of the opaque block from a null base, compiled for the
// host under the address and undefined-behaviour sanitizers.  No HIP runtime is linked: the few names the
// host code refers to are defined here, and the device check answers that there is no device, so nothing
// is launched.
//   localba_map_args_main          runs the checks, prints "ok"
//   localba_map_args_main sizes    prints the size of every struct of orbgpu_localba_map.h and some offsets
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/localba_map.hip"

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

#define EXPECT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "localba_map_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

static int sizes() {
    std::printf("orbgpu_map_mirror_ba %zu\n", sizeof(orbgpu_map_mirror_ba));
    std::printf("orbgpu_localba_gather_job %zu\n", sizeof(orbgpu_localba_gather_job));
    std::printf("orbgpu_localba_gather_result %zu\n", sizeof(orbgpu_localba_gather_result));
    std::printf("orbgpu_localba_job %zu\n", sizeof(orbgpu_localba_job));
    std::printf("ba.covis_all_offset %zu\n", offsetof(orbgpu_map_mirror_ba, covis_all_offset));
    std::printf("ba.kf_first %zu\n", offsetof(orbgpu_map_mirror_ba, kf_first));
    std::printf("ba.kp_obs %zu\n", offsetof(orbgpu_map_mirror_ba, kp_obs));
    std::printf("ba.obs_idx %zu\n", offsetof(orbgpu_map_mirror_ba, obs_idx));
    std::printf("result.n_fixed %zu\n", offsetof(orbgpu_localba_gather_result, n_fixed));
    std::printf("result.n_stereo %zu\n", offsetof(orbgpu_localba_gather_result, n_stereo));
    return 0;
}

struct GatherArgs {  // the seventeen pointers of the gather after the strides; p[i] = NULL takes one away
    void* p[17];
};

static int gather(int n, const orbgpu_map_mirror* m, const orbgpu_map_mirror_ba* b, int ks, int ps, int ms, int es,
                  const GatherArgs& a, const void* jobs) {
    return orbgpu_local_ba_gather_batch_device(
        n, static_cast<const orbgpu_localba_gather_job*>(jobs), m, b, ks, ps, ms, es, a.p[0],
        static_cast<orbgpu_localba_gather_result*>(a.p[1]), static_cast<orbgpu_localba_job*>(a.p[2]),
        static_cast<float*>(a.p[3]), static_cast<uint8_t*>(a.p[4]), static_cast<float*>(a.p[5]), static_cast<float*>(a.p[6]),
        static_cast<int*>(a.p[7]), static_cast<int*>(a.p[8]), static_cast<float*>(a.p[9]), static_cast<float*>(a.p[10]),
        static_cast<int*>(a.p[11]), static_cast<int*>(a.p[12]), static_cast<int*>(a.p[13]), static_cast<int*>(a.p[14]),
        static_cast<int*>(a.p[15]), nullptr);
}

struct CollectArgs {  // the eleven pointers of the collection a call needs, then Tcw_out, Xw_out, kf_Tcw, pos
    const void* in[9];
    void* out[2];
    float* kf_Tcw;
    float* pos;
};

static int collect(int n, int ks, int ms, int es, const CollectArgs& a, int n_kf, int n_pt) {
    return orbgpu_local_ba_collect_batch_device(
        n, static_cast<const orbgpu_localba_job*>(a.in[0]), ks, ms, es, static_cast<const float*>(a.in[1]),
        static_cast<const int*>(a.in[2]), static_cast<const int*>(a.in[3]), static_cast<const int*>(a.in[4]),
        static_cast<const int*>(a.in[5]), static_cast<const int*>(a.in[6]), static_cast<const uint8_t*>(a.in[7]),
        static_cast<const float*>(a.in[8]), static_cast<const float*>(a.in[8]), static_cast<int*>(a.out[0]),
        static_cast<int*>(a.out[1]), n_kf, n_pt, a.kf_Tcw, a.pos, nullptr);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    char block[256];
    void* p = block;  // never dereferenced: every call below returns before the device is looked at, or finds none
    auto cip = static_cast<const int*>(p);
    auto cfp = static_cast<const float*>(p);
    auto cbp = static_cast<const uint8_t*>(p);
    orbgpu_map_mirror full;
    std::memset(&full, 0, sizeof(full));
    full.n_kf = 4;
    full.n_pt = 9;
    full.n_slots_total = 12;
    full.n_obs_total = 12;
    full.kf_bad = cbp;
    full.slot_offset = full.n_slots = full.slots = cip;
    full.pt_flags = full.obs_offset = full.n_obs = full.obs = cip;
    full.pos = cfp;  // covis, children, parent, normal, desc and the distances are not read by the gather
    orbgpu_map_mirror_ba ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.n_covis_all_total = 5;
    ba.covis_all_offset = ba.n_covis_all = ba.covis_all = ba.obs_idx = cip;
    ba.kf_first = cbp;
    ba.kf_Tcw = ba.kf_cam = ba.kp_obs = ba.kp_inv_sigma2 = cfp;
    GatherArgs all;
    for (void*& q : all.p) q = p;
    EXPECT(gather(1, &full, &ba, 8, 8, 8, 8, all, p) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
    EXPECT(gather(-1, &full, &ba, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, &full, &ba, 0, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, &full, &ba, 8, 0, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, &full, &ba, 8, 8, 0, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, &full, &ba, 8, 8, 8, 0, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1 << 20, &full, &ba, 1 << 12, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1 << 20, &full, &ba, 8, 1 << 12, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1 << 20, &full, &ba, 8, 8, 1 << 12, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1 << 20, &full, &ba, 8, 8, 8, 1 << 12, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, nullptr, &ba, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, &full, nullptr, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    EXPECT(gather(1, &full, &ba, 8, 8, 8, 8, all, nullptr) == ORBGPU_ERR_ARG);
    for (int i = 0; i < 16; ++i) {
        GatherArgs a = all;
        a.p[i] = nullptr;
        EXPECT(gather(1, &full, &ba, 8, 8, 8, 8, a, p) == ORBGPU_ERR_ARG);
    }
    GatherArgs none;
    for (void*& q : none.p) q = nullptr;
    EXPECT(gather(0, nullptr, nullptr, 8, 8, 8, 8, none, nullptr) == ORBGPU_OK);  // nothing to do: no device needed
    // the mirrors: negative counts, and NULL arrays with positive counts
    for (int which = 0; which < 4; ++which) {
        orbgpu_map_mirror m = full;
        (which == 0 ? m.n_kf : which == 1 ? m.n_pt : which == 2 ? m.n_slots_total : m.n_obs_total) = -1;
        EXPECT(gather(1, &m, &ba, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    }
    {
        orbgpu_map_mirror_ba b = ba;
        b.n_covis_all_total = -1;
        EXPECT(gather(1, &full, &b, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    }
    const size_t read_by_gather[] = {offsetof(orbgpu_map_mirror, kf_bad),    offsetof(orbgpu_map_mirror, slot_offset),
                                     offsetof(orbgpu_map_mirror, n_slots),   offsetof(orbgpu_map_mirror, slots),
                                     offsetof(orbgpu_map_mirror, pt_flags),  offsetof(orbgpu_map_mirror, obs_offset),
                                     offsetof(orbgpu_map_mirror, n_obs),     offsetof(orbgpu_map_mirror, obs),
                                     offsetof(orbgpu_map_mirror, pos)};
    for (size_t off : read_by_gather) {
        orbgpu_map_mirror m = full;
        std::memset(reinterpret_cast<char*>(&m) + off, 0, sizeof(void*));
        EXPECT(gather(1, &m, &ba, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    }
    for (size_t off = offsetof(orbgpu_map_mirror_ba, covis_all_offset); off < sizeof(orbgpu_map_mirror_ba);
         off += sizeof(void*)) {
        orbgpu_map_mirror_ba b = ba;
        std::memset(reinterpret_cast<char*>(&b) + off, 0, sizeof(void*));
        EXPECT(gather(1, &full, &b, 8, 8, 8, 8, all, p) == ORBGPU_ERR_ARG);
    }
    orbgpu_map_mirror empty;  // no keyframes, no points: every array may be NULL
    std::memset(&empty, 0, sizeof(empty));
    orbgpu_map_mirror_ba empty_ba;
    std::memset(&empty_ba, 0, sizeof(empty_ba));
    EXPECT(gather(1, &empty, &empty_ba, 8, 8, 8, 8, all, p) == ORBGPU_ERR_NO_DEVICE);

    // the collection
    CollectArgs c;
    for (const void*& q : c.in) q = p;
    for (void*& q : c.out) q = p;
    c.kf_Tcw = c.pos = static_cast<float*>(p);
    EXPECT(collect(1, 8, 8, 8, c, 4, 9) == ORBGPU_ERR_NO_DEVICE);
    EXPECT(collect(-1, 8, 8, 8, c, 4, 9) == ORBGPU_ERR_ARG);
    EXPECT(collect(1, 0, 8, 8, c, 4, 9) == ORBGPU_ERR_ARG);
    EXPECT(collect(1, 8, 0, 8, c, 4, 9) == ORBGPU_ERR_ARG);
    EXPECT(collect(1, 8, 8, 0, c, 4, 9) == ORBGPU_ERR_ARG);
    EXPECT(collect(1, 8, 8, 8, c, -1, 9) == ORBGPU_ERR_ARG);
    EXPECT(collect(1, 8, 8, 8, c, 4, -1) == ORBGPU_ERR_ARG);
    EXPECT(collect(1 << 20, 8, 8, 1 << 12, c, 4, 9) == ORBGPU_ERR_ARG);
    for (int i = 0; i < 8; ++i) {
        CollectArgs a = c;
        a.in[i] = nullptr;
        EXPECT(collect(1, 8, 8, 8, a, 4, 9) == ORBGPU_ERR_ARG);
    }
    for (int i = 0; i < 2; ++i) {
        CollectArgs a = c;
        a.out[i] = nullptr;
        EXPECT(collect(1, 8, 8, 8, a, 4, 9) == ORBGPU_ERR_ARG);
    }
    {
        CollectArgs a = c;
        a.in[8] = nullptr;  // no Tcw_out / Xw_out: an error only with a mirror array to write
        EXPECT(collect(1, 8, 8, 8, a, 4, 9) == ORBGPU_ERR_ARG);
        a.kf_Tcw = a.pos = nullptr;
        EXPECT(collect(1, 8, 8, 8, a, 4, 9) == ORBGPU_ERR_NO_DEVICE);
    }
    CollectArgs cnone;
    std::memset(&cnone, 0, sizeof(cnone));
    EXPECT(collect(0, 8, 8, 8, cnone, 0, 0) == ORBGPU_OK);

    // the carving: sizes from a null base grow with every dimension and are 256-byte multiples
    size_t prev = 0;
    for (int n = 0; n <= 64; n += 8) {
        const size_t a = orbgpu_local_ba_gather_workspace_bytes(n, 10 * n, 100 * n);
        EXPECT(a > 0 && a % 256 == 0 && a >= prev);
        prev = a;
    }
    EXPECT(orbgpu_local_ba_gather_workspace_bytes(-5, -5, -5) == orbgpu_local_ba_gather_workspace_bytes(1, 1, 1));
    EXPECT(orbgpu_local_ba_gather_workspace_bytes(2, 0, 0) == orbgpu_local_ba_gather_workspace_bytes(2, 1, 1));
    EXPECT(orbgpu_local_ba_gather_workspace_bytes(1 << 20, 1 << 12, 4) == 0);  // n * n_kf does not fit an int
    EXPECT(orbgpu_local_ba_gather_workspace_bytes(1 << 20, 4, 1 << 12) == 0);
    std::printf("ok\n");
    return 0;
}
